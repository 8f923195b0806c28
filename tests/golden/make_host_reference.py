"""Writes tests/golden/host_reference.json: what the upstream OpenP5 host modules (src/src_t5 of the original repository) return on
the inputs of tests/test_host.py's `*_equals_reference` tests -- whole-word ids (processor/Collator.py), the generation trie
(utils/generation_trie.py), the metrics (utils/evaluate.py), datasets and the distributed sampler (data/*.py,
processor/DistMultiDataTaskSampler.py).  The tests compare this package against the stored answers, so they need no upstream checkout.

    python tests/golden/make_host_reference.py <path to the upstream repository's src/src_t5>
"""
import importlib
import json
import os
import random
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "host_reference.json")


def whole_word_ids(ref, tok):
    rnd = random.Random(0)
    cases = []
    for _ in range(50):
        n = rnd.randint(2, 30)
        ids = [rnd.randint(3, 400) for _ in range(n)] + [1] + [0] * rnd.randint(0, 5)
        cases.append({"ids": ids, "whole_word_ids": ref.calculate_whole_word_ids(tok.convert_ids_to_tokens(ids), ids)})
    return cases


def trie(gt):
    rnd = random.Random(1)
    seqs = [[0] + [rnd.randint(2, 9) for _ in range(rnd.randint(1, 5))] + [1] for _ in range(200)]
    t = gt.Trie(seqs)
    queries = []
    for _ in range(500):
        pre = rnd.choice(seqs)[: rnd.randint(0, 6)]
        queries.append({"prefix": pre, "allowed": sorted(t.get(pre))})
    return {"sequences": seqs, "len": len(t), "queries": queries}


def metrics(ref):
    rnd = random.Random(2)
    k, B = 10, 30
    preds = [f"i{rnd.randint(0, 40)}" for _ in range(B * k)]
    gold = [f"i{rnd.randint(0, 40)}" for _ in range(B)]
    scores = [rnd.random() for _ in range(B * k)]
    ms = ['hit@5', 'hit@10', 'ndcg@5', 'ndcg@10']
    rel = ref.rel_results(preds, gold, scores, k)
    positive = {f"u{b}": sorted(set(rnd.sample(preds, 5))) for b in range(B)}
    id2user = {b: f"u{b}" for b in range(B)}
    filtered = ref.rel_results_filtered({u: set(v) for u, v in positive.items()}, id2user, list(range(B)), k, preds, gold, scores, 5)
    return {"k": k, "predictions": preds, "gold": gold, "scores": scores, "metrics": ms, "rel_results": rel,
            "metrics_results": [float(x) for x in ref.get_metrics_results(rel, ms)], "positive": positive,
            "filter_k": 5, "rel_results_filtered": filtered}


def dataset_and_sampler(RD, RT, RS):
    from torch.utils.data import ConcatDataset
    from tests.test_host import make_args
    with tempfile.TemporaryDirectory() as tmp:
        args = make_args(tmp)
        args.test_filtered = 0
        random.seed(5)
        ds = RD.MultiTaskDataset(args, "Toy", "train")
        td = RT.TestDataset(args, "Toy", "straightforward")
        out = {"train_input": ds.data["input"], "train_output": ds.data["output"], "task_index": ds.task_index, "item_map": ds.item_map,
               "test_data": td.data, "test_all_items": td.all_items, "sampler": []}
        for epoch in (0, 1):
            s = RS.DistMultiDataTaskSampler(ConcatDataset([ds]), 4, 2, 1, seed=2023)
            s.set_epoch(epoch)
            out["sampler"].append({"epoch": epoch, "indices": [int(i) for i in iter(s)], "len": len(s)})
    return out


def main():
    src = os.path.abspath(sys.argv[1])
    sys.dont_write_bytecode = True
    sys.path.append(src)
    from openp5_amd.tokenizer import build_offline_tokenizer
    ref = {"whole_word_ids": whole_word_ids(importlib.import_module("processor.Collator"), build_offline_tokenizer()),
           "trie": trie(importlib.import_module("utils.generation_trie")),
           "metrics": metrics(importlib.import_module("utils.evaluate")),
           "dataset_and_sampler": dataset_and_sampler(importlib.import_module("data.MultiTaskDataset"), importlib.import_module("data.TestDataset"),
                                                      importlib.import_module("processor.DistMultiDataTaskSampler"))}
    with open(OUT, "w") as f:
        json.dump(ref, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
