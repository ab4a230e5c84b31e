#!/usr/bin/env python3
"""Time of the document-collection entry points (sa_doc_array_device,
sa_doc_frequency_device, sa_doc_list_device) on one MI355X, next to what a
device caller writes without them in plain torch on the same GPU:

    DA        torch.searchsorted(doc_off, sa, right=True) - 1
    DA + PRV  the same, a stable torch.sort by document, one scatter of neighbours
    df, list  repeat_interleave for the query ids, a gather of DA, and
              torch.unique of the 64-bit keys (query << 32 | document)

Those torch expressions are the baseline, not the code under test.

The text is random DNA generated on the device (2^24 and 2^28 bytes by
default), its SA built in place, cut into D = 16, 4096 and 2^20 documents at
seeded random places.  The intervals come from sa_find_device: 2^20 patterns of
12 bytes cut from the text (short intervals) and 64 patterns of 4 bytes (long
ones).  For each measurement the outputs are compared first, then the calls
are warmed up and timed alone between two device events, --runs times,
alternating run by run.  Reported per call: median, minimum and maximum in ms.
Prints one JSON line and writes it to --out when given.  With no GPU the
script fails.

    python scripts/bench_docs.py [--n 16777216 268435456] [--docs 16 4096 1048576] [--runs 10] [--out profiles/bench_docs.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BATCHES = {"short": (1 << 20, 12), "long": (64, 4)}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1 << 24, 1 << 28])
    ap.add_argument("--docs", type=int, nargs="+", default=[16, 4096, 1 << 20])
    ap.add_argument("--batches", nargs="+", default=list(BATCHES), choices=sorted(BATCHES))
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-torch", action="store_true", help="no baseline, no comparison (kernel traces)")
    ap.add_argument("--out", default=None)
    return ap.parse_args()


def timed(torch, fns, runs, warmup):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    for _ in range(runs):
        for name, fn in fns.items():
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    return {name: {"ms_median": float(np.median(v)), "ms_min": min(v), "ms_max": max(v), "runs": runs}
            for name, v in ms.items()}


def torch_da(torch, d_sa, d_off):
    return torch.searchsorted(d_off, d_sa.to(torch.int64), right=True) - 1


def torch_da_prev(torch, d_sa, d_off):
    da = torch_da(torch, d_sa, d_off)
    srt, order = torch.sort(da, stable=True)
    prev = torch.zeros_like(da)
    same = srt[1:] == srt[:-1]
    prev[order[1:][same]] = order[:-1][same] + 1
    return da, prev


def torch_docs(torch, d_da, d_lo, d_hi):
    """(df, offsets, ids) by the expression a device caller writes today."""
    lo = d_lo.to(torch.int64)
    cnt = d_hi.to(torch.int64) - lo
    nq = cnt.numel()
    off = torch.zeros(nq + 1, dtype=torch.int64, device=cnt.device)
    torch.cumsum(cnt, 0, out=off[1:])
    qid = torch.repeat_interleave(torch.arange(nq, device=cnt.device), cnt)
    idx = lo[qid] + (torch.arange(qid.numel(), device=cnt.device) - off[qid])
    keys = torch.unique((qid << 32) | d_da[idx].to(torch.int64))
    df = torch.bincount(keys >> 32, minlength=nq)
    doff = torch.zeros(nq + 1, dtype=torch.int64, device=cnt.device)
    torch.cumsum(df, 0, out=doff[1:])
    return df, doff, keys & 0xFFFFFFFF


def bench_collection(torch, a, b, d_text, d_sa, n, D, ivals):
    dev = d_text.device
    sptr = torch.cuda.current_stream(dev).cuda_stream
    g = torch.Generator(device=dev).manual_seed(a.seed + D)
    d_off = torch.zeros(D + 1, dtype=torch.int64, device=dev)
    d_off[1:D] = torch.sort(torch.randint(0, n + 1, (D - 1,), generator=g, device=dev)).values
    d_off[D] = n
    d_da = torch.empty(n, dtype=torch.int32, device=dev)
    d_prev = torch.empty(n, dtype=torch.int32, device=dev)
    rec = {"D": D, "array": {}, "queries": {}}

    fns = {"da": lambda: b.doc_array(n, d_sa, d_off, D, d_da, None, stream=sptr),
           "da_prev": lambda: b.doc_array(n, d_sa, d_off, D, d_da, d_prev, stream=sptr)}
    fns["da_prev"]()
    if not a.skip_torch:
        wda, wprev = torch_da_prev(torch, d_sa, d_off)
        assert torch.equal(d_da.to(torch.int64), wda), "DA differs from the torch expression"
        assert torch.equal(d_prev.to(torch.int64), wprev), "PRV differs from the torch expression"
        del wda, wprev
        fns["torch_da"] = lambda: torch_da(torch, d_sa, d_off)
        fns["torch_da_prev"] = lambda: torch_da_prev(torch, d_sa, d_off)
    rec["array"] = timed(torch, fns, a.runs, a.warmup)
    torch.cuda.empty_cache()

    for name, (d_lo, d_hi) in ivals.items():
        nq = d_lo.numel()
        d_df = torch.empty(nq, dtype=torch.int32, device=dev)
        d_qoff = torch.empty(nq + 1, dtype=torch.int64, device=dev)
        total = b.doc_list(n, d_da, d_prev, d_lo, d_hi, nq, d_qoff, None, 0, stream=sptr)
        d_ids = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        ranks = int((d_hi.to(torch.int64) - d_lo.to(torch.int64)).sum())
        fns = {"frequency": lambda: b.doc_frequency(n, d_prev, d_lo, d_hi, nq, d_df, stream=sptr),
               "list": lambda: b.doc_list(n, d_da, d_prev, d_lo, d_hi, nq, d_qoff, d_ids, total, stream=sptr),
               "list_rank_order": lambda: b.doc_list(n, d_da, d_prev, d_lo, d_hi, nq, d_qoff, d_ids, total,
                                                     order="rank", stream=sptr)}
        fns["frequency"]()
        fns["list"]()
        if not a.skip_torch:
            wdf, woff, wids = torch_docs(torch, d_da, d_lo, d_hi)
            assert torch.equal(d_df.to(torch.int64), wdf), "df differs from the torch expression"
            assert torch.equal(d_qoff, woff), "offsets differ from the torch expression"
            assert torch.equal(d_ids[:total].to(torch.int64), wids), "ids differ from the torch expression"
            del wdf, woff, wids
            fns["torch"] = lambda: torch_docs(torch, d_da, d_lo, d_hi)
        r = timed(torch, fns, a.runs, a.warmup)
        r.update({"nq": nq, "ranks": ranks, "ids": total})
        r["frequency_gb_per_s"] = ranks * 4 / (r["frequency"]["ms_median"] * 1e6)
        rec["queries"][name] = r
        torch.cuda.empty_cache()
    return rec


def bench_text(torch, a, n):
    from hpc_suffix_array_amd import DeviceBuilder
    dev = torch.device("cuda", 0)
    b = DeviceBuilder(n)
    d_text = torch.empty(n, dtype=torch.uint8, device=dev)
    b.generate_text(d_text, n, b"ACGT", seed=a.seed)
    d_sa = torch.empty(n, dtype=torch.int32, device=dev)
    st = b.build(d_text, n, d_sa)
    torch.cuda.synchronize()
    sptr = torch.cuda.current_stream(dev).cuda_stream
    ivals = {}
    for name in a.batches:
        nq, m = BATCHES[name]
        g = torch.Generator(device=dev).manual_seed(a.seed + nq)
        start = torch.randint(0, n - m, (nq,), generator=g, device=dev)
        d_pat = d_text[(start[:, None] + torch.arange(m, device=dev)[None, :]).reshape(-1)].contiguous()
        d_poff = (torch.arange(nq + 1, device=dev, dtype=torch.int64) * m).contiguous()
        d_lo = torch.empty(nq, dtype=torch.int32, device=dev)
        d_hi = torch.empty(nq, dtype=torch.int32, device=dev)
        b.find(d_text, n, d_sa, d_pat, nq * m, d_poff, nq, d_lo, d_hi, stream=sptr)
        torch.cuda.synchronize()
        ivals[name] = (d_lo, d_hi)
    out = {"n": n, "build_ms": st["total_ms"], "collections": []}
    for D in a.docs:
        if D <= n:
            out["collections"].append(bench_collection(torch, a, b, d_text, d_sa, n, D, ivals))
    b.close()
    return out


def main():
    a = parse()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_docs.py needs an MI355X: no HIP device is visible")
    from hpc_suffix_array_amd import _native as N
    out = {"bench": "docs", "kind": "dna", "seed": a.seed, "tile": N.DOC_TILE, "group_max": N.DOC_GROUP_MAX,
           "src_hash": N.source_hash(), "cus": torch.cuda.get_device_properties(0).multi_processor_count,
           "texts": [bench_text(torch, a, n) for n in a.n]}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
