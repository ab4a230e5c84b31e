#!/usr/bin/env python3
"""Time of the batched locate (sa_locate_device) on one MI355X, next to what a
device caller writes without it: torch.repeat_interleave for the query ids, a
gather of the SA, and torch.sort of the 64-bit keys (query << 32 | position).
That torch expression is the baseline, not the code under test.

The text is random DNA (2^28 by default), generated on the device, its SA
built in place; the patterns are cut from the text and their intervals come
from sa_find_device.  Batches:

    a   2^20 patterns of 16 bytes   mostly one hit
    b   2^20 patterns of 12 bytes   about 16 hits
    c   2^16 patterns of 8 bytes    about 4096 hits: across the class boundary
    d   64 patterns of 4 bytes      about 2^20 hits each: the large class

For each batch and each order (text, sa) the outputs are compared first
(offsets and positions equal), then the calls are warmed up and timed alone
between two device events, --runs times (at least 20), alternating run by run:

    locate       one call with the output allocated (pos_cap = the total)
    two_call     the sizing call, torch.empty, the writing call
    torch        the torch expression (the SA order leaves its sort out)

Reported per call: median, minimum and maximum in ms and ns per hit.  The
condition (batches a and b): the locate median is below the torch median by
more than the larger of the two ranges (max - min).  Prints one JSON line and
writes it to --out when given.  With no GPU the script fails.

    python scripts/bench_locate.py [--n 268435456] [--batches a b c d] [--runs 20] [--out profiles/bench_locate.json]
    python scripts/bench_locate.py --batches b --runs 1 --warmup 0 --skip-torch     # one run for a kernel trace
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

BATCHES = {"a": (1 << 20, 16), "b": (1 << 20, 12), "c": (1 << 16, 8), "d": (64, 4)}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 28)
    ap.add_argument("--batches", nargs="+", default=list(BATCHES), choices=sorted(BATCHES))
    ap.add_argument("--orders", nargs="+", default=["text", "sa"], choices=["text", "sa"])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--runs", type=int, default=20)
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


def torch_locate(torch, d_sa, d_lo, d_hi, order):
    """(offsets, positions) by the expression a device caller writes today."""
    lo = d_lo.to(torch.int64) & 0xFFFFFFFF
    cnt = (d_hi.to(torch.int64) & 0xFFFFFFFF) - lo
    off = torch.zeros(cnt.numel() + 1, dtype=torch.int64, device=cnt.device)
    torch.cumsum(cnt, 0, out=off[1:])
    qid = torch.repeat_interleave(torch.arange(cnt.numel(), device=cnt.device), cnt)
    idx = lo[qid] + (torch.arange(qid.numel(), device=cnt.device) - off[qid])
    pos = d_sa[idx].to(torch.int64) & 0xFFFFFFFF
    if order == "sa":
        return off, pos
    keys = torch.sort((qid << 32) | pos).values
    return off, keys & 0xFFFFFFFF


def one(torch, a, b, d_text, d_sa, name):
    n = a.n
    dev = d_text.device
    nq, m = BATCHES[name]
    g = torch.Generator(device=dev).manual_seed(a.seed + ord(name))
    start = torch.randint(0, n - m, (nq,), generator=g, device=dev)
    d_pat = d_text[(start[:, None] + torch.arange(m, device=dev)[None, :]).reshape(-1)].contiguous()
    d_poff = (torch.arange(nq + 1, device=dev, dtype=torch.int64) * m).contiguous()
    d_lo = torch.empty(nq, dtype=torch.int32, device=dev)
    d_hi = torch.empty(nq, dtype=torch.int32, device=dev)
    sptr = torch.cuda.current_stream(dev).cuda_stream
    b.find(d_text, n, d_sa, d_pat, nq * m, d_poff, nq, d_lo, d_hi, stream=sptr)
    torch.cuda.synchronize()
    d_off = torch.empty(nq + 1, dtype=torch.int64, device=dev)
    total = b.locate(n, d_sa, d_lo, d_hi, nq, d_off, None, 0, stream=sptr)
    d_pos = torch.empty(total, dtype=torch.int32, device=dev)
    cnt = ((d_hi.to(torch.int64) & 0xFFFFFFFF) - (d_lo.to(torch.int64) & 0xFFFFFFFF))
    large = int((cnt > N_TILE).sum())
    rec = {"batch": name, "nq": nq, "pattern_bytes": m, "hits": total, "large_queries": large,
           "largest_query": int(cnt.max()), "orders": {}}
    del cnt
    for order in a.orders:
        def locate():
            b.locate(n, d_sa, d_lo, d_hi, nq, d_off, d_pos, total, order=order, stream=sptr)

        def two_call():
            t = b.locate(n, d_sa, d_lo, d_hi, nq, d_off, None, 0, order=order, stream=sptr)
            p = torch.empty(t, dtype=torch.int32, device=dev)
            b.locate(n, d_sa, d_lo, d_hi, nq, d_off, p, t, order=order, stream=sptr)

        fns = {"locate": locate, "two_call": two_call}
        if not a.skip_torch:
            # the outputs agree before anything is timed
            d_pos.fill_(-1)
            locate()
            woff, wpos = torch_locate(torch, d_sa, d_lo, d_hi, order)
            assert torch.equal(d_off, woff), "offsets differ from the torch expression"
            assert torch.equal(d_pos.to(torch.int64) & 0xFFFFFFFF, wpos), "positions differ from the torch expression"
            del woff, wpos
            fns["torch"] = lambda: torch_locate(torch, d_sa, d_lo, d_hi, order)
        r = timed(torch, fns, a.runs if a.skip_torch else max(20, a.runs), a.warmup)
        for v in r.values():
            v["ns_per_hit_median"] = v["ms_median"] * 1e6 / max(total, 1)
        if not a.skip_torch:
            spread = max(r["locate"]["ms_max"] - r["locate"]["ms_min"], r["torch"]["ms_max"] - r["torch"]["ms_min"])
            r["larger_range_ms"] = spread
            r["locate_over_torch_median"] = r["locate"]["ms_median"] / r["torch"]["ms_median"]
            r["below_torch_by_more_than_the_range"] = bool(
                r["torch"]["ms_median"] - r["locate"]["ms_median"] > spread)
        rec["orders"][order] = r
        torch.cuda.empty_cache()
    return rec


def main():
    global N_TILE
    a = parse()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_locate.py needs an MI355X: no HIP device is visible")
    from hpc_suffix_array_amd import DeviceBuilder, _native as N
    N_TILE = N.LOCATE_TILE
    dev = torch.device("cuda", 0)
    b = DeviceBuilder(a.n)
    d_text = torch.empty(a.n, dtype=torch.uint8, device=dev)
    b.generate_text(d_text, a.n, b"ACGT", seed=a.seed)
    d_sa = torch.empty(a.n, dtype=torch.int32, device=dev)
    st = b.build(d_text, a.n, d_sa)
    torch.cuda.synchronize()
    out = {"bench": "locate", "n": a.n, "kind": "dna", "seed": a.seed, "tile": N.LOCATE_TILE,
           "src_hash": N.source_hash(), "cus": torch.cuda.get_device_properties(0).multi_processor_count,
           "build_ms": st["total_ms"], "results": []}
    for name in a.batches:
        out["results"].append(one(torch, a, b, d_text, d_sa, name))
    if not a.skip_torch:
        out["condition_met"] = {r["batch"]: {o: v["below_torch_by_more_than_the_range"]
                                             for o, v in r["orders"].items()}
                                for r in out["results"] if r["batch"] in ("a", "b")}
    b.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
