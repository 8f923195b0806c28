"""Cases of the wide beam search (csrc/p5_decode_wide.h) shared by tests/test_wide_beams_emu.py (host emulation) and
tests/test_gpu_wide_beams.py (MI355X)."""
import pytest
import torch

from oracle import t5_oracle as O
from openp5_amd.trie import Trie, prefix_allowed_tokens_fn
from tests import cases


def gen_pair(be, ocfg, B, L, K, max_len, n_items, params_fn=None, wide_max_rows=None, dtype="fp32", mode=None, seed=5, model=None):
    """one generate() call on a fresh model (or `model`) over make_items(n_items): (output dict, model)"""
    params = O.init_params(ocfg, 7)
    if params_fn is not None:
        params = params_fn(params, ocfg)
    m = model or cases.build_model(be, ocfg, params, dtype)
    m.eval()
    if mode is not None:
        m.generation_mode = mode
    if wide_max_rows is not None:
        m.wide_max_rows = wide_max_rows
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, L, 4, seed)
    items = cases.make_items(n_items, seed, hi=min(60, ocfg.vocab_size - 1))
    out = m.generate(input_ids=ids, attention_mask=mask, whole_word_ids=ww, max_length=max_len,
                     prefix_allowed_tokens_fn=prefix_allowed_tokens_fn(Trie(items)), num_beams=K, num_return_sequences=K,
                     output_scores=True, return_dict_in_generate=True)
    out["items"], out["params"] = items, params
    return out, m


def tie_heavy_params(params, ocfg):
    """embedding rows 7 .. 60 (every item token) identical: the children of a beam tie exactly, the order among them is the key's"""
    p = dict(params)
    E = p["shared.weight"].clone()
    E[7:61] = E[7]
    p["shared.weight"] = E
    return p


def narrow_vs_wide_case(be, ocfg, B, L, K, max_len, n_items, params_fn=None):
    """K <= 64: the narrow step and the wide step (p5_set_option gen_wide 1) return the same sequences and scores, bit for bit."""
    params = O.init_params(ocfg, 7)
    m = cases.build_model(be, ocfg, params_fn(params, ocfg) if params_fn else params, "fp32")
    a, _ = gen_pair(be, ocfg, B, L, K, max_len, n_items, params_fn=params_fn, model=m)
    be.check(be.lib.p5_set_option(b"gen_wide", 1), "p5_set_option")
    try:
        b, _ = gen_pair(be, ocfg, B, L, K, max_len, n_items, params_fn=params_fn, model=m)
    finally:
        be.lib.p5_set_option(b"gen_wide", 0)
    assert torch.equal(a["sequences"].cpu(), b["sequences"].cpu()), "narrow and wide sequences differ"
    assert torch.equal(a["sequences_scores"].cpu(), b["sequences_scores"].cpu()), "narrow and wide scores differ"
    return a


def check_leaves(seq, score, K, items, eos=1):
    """per item: the live hypotheses (score > -1e8) are distinct, complete items of the trie, in non-increasing score order"""
    valid = {tuple(it) for it in items}
    seq, score = seq.cpu(), score.cpu()
    B = seq.shape[0] // K
    for b in range(B):
        sc = score[b * K:(b + 1) * K]
        assert bool((sc[1:] <= sc[:-1]).all()), f"item {b}: scores not sorted"
        seen = set()
        for k in range(K):
            if float(sc[k]) <= -1e8:
                continue
            row = seq[b * K + k].tolist()
            assert eos in row, f"item {b} beam {k}: unfinished hypothesis {row}"
            h = tuple(row[:row.index(eos) + 1])
            assert h in valid, f"item {b} beam {k}: {h} is not an item of the trie"
            assert h not in seen, f"item {b}: {h} returned twice"
            seen.add(h)


def wide_leaves_case(be, ocfg, B, L, K, max_len, n_items):
    out, _ = gen_pair(be, ocfg, B, L, K, max_len, n_items)
    check_leaves(out["sequences"], out["sequences_scores"], K, out["items"])
    return out


def oracle_case(be, ocfg, B, L, K, max_len, n_items, score_tol=2e-5, dtype="fp32", mode=None, tie_tol=0.0):
    """generate() against O.beam_search at the same width (token-exact, scores within score_tol; tie_tol > 0 for the bf16 search)"""
    out, _ = gen_pair(be, ocfg, B, L, K, max_len, n_items, dtype=dtype, mode=mode)
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, L, 4, 5)
    trie = Trie(out["items"])
    with torch.no_grad():
        s_ref, sc_ref = O.beam_search(out["params"], ocfg, ids, ww, mask, lambda b, s: trie.get(s.tolist()), K, max_len)
    cases.compare_generation(out["sequences"].cpu(), out["sequences_scores"].cpu(), s_ref, sc_ref, score_tol, tie_tol=tie_tol, K=K)
    return out


def runner_widened_case(be, tmp_path, id_metrics):
    """--test_filtered 1 --test_filtered_batch 1 on a toy dataset whose longest history makes the width > 64; the metrics equal
    O.beam_search at that width + evaluate.rel_results_filtered + get_metrics_results (DistributedRunner.py:204-269 restated)."""
    import random
    from torch.utils.data import ConcatDataset, DataLoader
    from openp5_amd import evaluate
    from openp5_amd.collator import Collator
    from openp5_amd.data import MultiTaskDataset
    from openp5_amd.runner import DistributedRunner
    from openp5_amd.sampler import SingleMultiDataTaskSampler
    from openp5_amd.tokenizer import build_offline_tokenizer
    from tests.test_host import make_args
    tmp_path.mkdir(parents=True, exist_ok=True)
    tok = build_offline_tokenizer(2400)
    args = make_args(str(tmp_path), ["--epochs", "1", "--test_before_train", "0", "--test_epoch", "0", "--metrics", "hit@1,hit@5,ndcg@5",
                                     "--batch_size", "8", "--sample_num", "1,1", "--max_his", "8", "--eval_batch_size", "3",
                                     "--test_filtered", "1", "--test_filtered_batch", "1", "--id_metrics", id_metrics],
                     toy=dict(n_users=4, n_items=90, n_inter=4 * 75))
    random.seed(0)
    train = ConcatDataset([MultiTaskDataset(args, "Toy", "train")])
    loader = DataLoader(train, sampler=SingleMultiDataTaskSampler(train, args.batch_size, args.seed), batch_size=args.batch_size,
                        collate_fn=Collator(tok))
    ocfg = O.T5Cfg(vocab_size=len(tok), d_model=64, d_ff=128, num_layers=1, num_decoder_layers=1, num_heads=1)
    params = O.init_params(ocfg, 11)
    model = cases.build_model(be, ocfg, params, "fp32")
    r = DistributedRunner(model, tok, loader, None, torch.device("cpu") if be.is_emulator else be.device, args, 0)
    got = r.test()
    widths = []
    for li, tl in enumerate(r.testloaders):
        ds = tl.dataset
        width = r.generate_num + ds.max_positive
        widths.append(width)
        trie, _, _ = r._dataset_trie(ds)
        res, total = 0, 0
        for batch in tl:
            with torch.no_grad():
                s_ref, sc_ref = O.beam_search(params, ocfg, batch[0], batch[2], batch[1], lambda b, s: trie.get(s.tolist()), width, 30)
            gold = tok.batch_decode(batch[3], skip_special_tokens=True)
            gen = tok.batch_decode(s_ref, skip_special_tokens=True)
            rel = evaluate.rel_results_filtered(ds.positive_text, ds.id2user, batch[5].numpy(), width, gen, gold, sc_ref.tolist(), r.generate_num)
            total += len(rel)
            res = res + evaluate.get_metrics_results(rel, r.metrics)
        want = dict(zip(r.metrics, (torch.as_tensor(res, dtype=torch.float64) / total).tolist()))
        assert got[li] == pytest.approx(want, abs=1e-12), (li, got[li], want)
    assert max(widths) > 64, widths
    return got
