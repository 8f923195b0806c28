"""Generates tests/golden/peaked_tiny.pt: a toy T5 TRAINED (oracle functions under torch autograd, seeded, CPU) to put real probability
mass on the tokens of an item trie -- the fixture of the pruned-ranking tests (tests/prune_cases.py).  Pruning by a score bound only
happens on such a model: a random-init one spreads its mass over the vocabulary, every prefix stays within reach of the N-th item and
92 % of the trie's rows or more are kept.

The task: the user's first input token decides a "home" item, the target is the home item shifted by 17 x Geometric(0.35) positions in the
catalogue -- a distribution with a clear head (so the top of the list is separated) and a tail (so rank 10 is not noise).

    python tests/golden/make_peaked_tiny.py          # about 2.5 minutes on 16 threads
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from oracle import t5_oracle as O          # noqa: E402
from tests.cases import make_items         # noqa: E402

CFG = dict(vocab_size=128, d_model=64, d_ff=128, num_layers=1, num_decoder_layers=1, num_heads=1)
N_ITEMS, ITEM_SEED, ITEM_HI = 300, 5, 60
L, BATCH, STEPS, LR, SEED = 12, 64, 1200, 5e-3, 2023


def train_batch(cfg, items_t, g):
    """inputs drawn as tests.cases.synth_batch draws them (padded rows, whole-word ids), labels = the target item's tokens behind the start"""
    ids = torch.randint(3, cfg.vocab_size, (BATCH, L), generator=g)
    mask = torch.ones(BATCH, L, dtype=torch.long)
    for b in range(1, BATCH):
        n = max(1, int(torch.randint(L // 2, L + 1, (1,), generator=g)))
        mask[b, n:] = 0
        ids[b, n:] = 0
    ww = torch.cumsum((torch.rand(BATCH, L, generator=g) < 0.4).long(), 1) * mask
    geo = torch.floor(torch.log(torch.rand(BATCH, generator=g).clamp_min(1e-12)) / torch.log(torch.tensor(0.65))).long()      # P(k) = 0.35 x 0.65^k
    target = ((ids[:, 0] * 7) % N_ITEMS + 17 * geo) % N_ITEMS
    labels = items_t[target][:, 1:]
    return ids, ww, mask, labels


def main():
    torch.manual_seed(SEED)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    cfg = O.T5Cfg(**CFG)
    items = make_items(N_ITEMS, ITEM_SEED, hi=ITEM_HI)
    T = max(len(q) for q in items)
    items_t = torch.zeros(len(items), T, dtype=torch.int64)
    for i, q in enumerate(items):
        items_t[i, :len(q)] = torch.tensor(q)
    P = {k: v.clone().requires_grad_(True) for k, v in O.init_params(cfg, 7).items()}
    opt = torch.optim.Adam(list(P.values()), lr=LR)
    g = torch.Generator().manual_seed(SEED)
    loss = None
    for step in range(STEPS):
        ids, ww, mask, labels = train_batch(cfg, items_t, g)
        nll = O.p5_forward_nll(P, cfg, ids, ww, mask, labels).view(BATCH, -1)
        is_eos = labels == cfg.eos_id
        n = is_eos.float().argmax(dim=1) + 1                       # (every item ends with </s>)
        keep = (torch.arange(labels.shape[1])[None, :] < n[:, None]).float()
        loss = (nll * keep).sum() / keep.sum()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        if step % 100 == 0 or step == STEPS - 1:
            print(f"step {step}: loss per token {float(loss):.4f}", flush=True)
    fx = dict(cfg=CFG, params={k: v.detach().clone() for k, v in P.items()}, n_items=N_ITEMS, item_seed=ITEM_SEED, item_hi=ITEM_HI, L=L,
              recipe=dict(batch=BATCH, steps=STEPS, lr=LR, seed=SEED, init_seed=7), final_loss=float(loss))
    torch.save(fx, os.path.join(HERE, "peaked_tiny.pt"))
    print("saved", os.path.getsize(os.path.join(HERE, "peaked_tiny.pt")), "bytes")


if __name__ == "__main__":
    main()
