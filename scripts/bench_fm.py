#!/usr/bin/env python3
"""Time and size of the FM-index (sa_fm_build_device / sa_fm_count_device /
sa_fm_locate_device) on one MI355X, next to the suffix-array queries that
answer the same questions with the text and the whole SA in HBM
(sa_find_device / sa_locate_device), in the same session on the same queries.

The text is random DNA (2^28 by default), generated on the device; its SA and
BWT are built there.  Reported:

    build     sa_fm_build_device at sa_sample = 32 (host clock round the call
              and a synchronise: it has one host wait inside), index bytes / n
    count     2^20 patterns of 12 / 32 / 128 bytes cut from the text:
              sa_fm_count_device and sa_find_device between two device events,
              alternating run by run; patterns per second; the intervals are
              compared first (the patterns occur, so they must be equal)
    locate    the intervals of the 12-byte patterns (about 16 hits each):
              sa_fm_locate_device and sa_locate_device with the output
              allocated, host clock (both wait for the stream), ns per hit;
              positions compared first

Every figure is the median of --runs runs after --warmup warm-up runs, with
the minimum and maximum beside it.  No ratio is asserted: backward search does
2 m dependent gathers where find does about 2 log2 n, and the claim of the
index is its memory.  Prints one JSON line and writes it to --out when given.
With no GPU the script fails.

    python scripts/bench_fm.py [--n 268435456] [--nq 1048576] [--runs 9] [--out profiles/bench_fm.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LENGTHS = (12, 32, 128)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 28)
    ap.add_argument("--nq", type=int, default=1 << 20)
    ap.add_argument("--sa-sample", type=int, default=32)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    return ap.parse_args()


def stats(v):
    return {"ms_median": float(np.median(v)), "ms_min": float(min(v)), "ms_max": float(max(v)), "runs": len(v)}


def timed_events(torch, fns, runs, warmup):
    """Each fn enqueues on the current stream: device events, alternating."""
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
    return {name: stats(v) for name, v in ms.items()}


def timed_host(torch, fns, runs, warmup):
    """Each fn waits for the device itself: the host clock between two synchronises."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    ms = {name: [] for name in fns}
    for _ in range(runs):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    return {name: stats(v) for name, v in ms.items()}


def u32(torch, x):
    return x.to(torch.int64) & 0xFFFFFFFF


def main():
    a = parse()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_fm.py needs an MI355X: no HIP device is visible")
    from hpc_suffix_array_amd import DeviceBuilder, _native as N
    dev = torch.device("cuda", 0)
    n, nq, s = a.n, a.nq, a.sa_sample
    b = DeviceBuilder(n)
    sptr = torch.cuda.current_stream(dev).cuda_stream
    d_text = torch.empty(n, dtype=torch.uint8, device=dev)
    b.generate_text(d_text, n, b"ACGT", seed=a.seed)
    d_sa = torch.empty(n, dtype=torch.int32, device=dev)
    st = b.build(d_text, n, d_sa)
    d_bwt = torch.empty(n, dtype=torch.uint8, device=dev)
    d_stats = torch.zeros(N.BWT_STATS, dtype=torch.int64, device=dev)
    b.bwt(d_text, n, d_sa, d_bwt, d_stats)
    torch.cuda.synchronize()
    primary = int(d_stats[0])
    cap = b.fm_index_bytes(n, s)
    d_index = torch.empty(cap, dtype=torch.uint8, device=dev)
    info = {}

    def build():
        info.update(b.fm_build(d_bwt, n, primary, d_index, cap, d_sa, s, stream=sptr))

    out = {"bench": "fm", "n": n, "kind": "dna", "seed": a.seed, "sa_sample": s, "nq": nq,
           "src_hash": N.source_hash(), "cus": torch.cuda.get_device_properties(0).multi_processor_count,
           "sa_build_ms": st["total_ms"]}
    out["build"] = timed_host(torch, {"fm_build": build}, a.runs, a.warmup)["fm_build"]
    out["index"] = dict(info, bytes_allocated=cap, bytes_per_n=info["bytes"] / n,
                        sa_and_text_bytes_per_n=5.0)
    ib = info["bytes"]
    g = torch.Generator(device=dev).manual_seed(a.seed + 7)
    out["count"] = []
    keep = None
    for m in LENGTHS:
        start = torch.randint(0, n - m, (nq,), generator=g, device=dev)
        d_pat = d_text[(start[:, None] + torch.arange(m, device=dev)[None, :]).reshape(-1)].contiguous()
        d_poff = (torch.arange(nq + 1, device=dev, dtype=torch.int64) * m).contiguous()
        lo_f, hi_f, lo_s, hi_s = (torch.full((nq,), -1, dtype=torch.int32, device=dev) for _ in range(4))

        def fm_count():
            b.fm_count(d_index, ib, d_pat, nq * m, d_poff, nq, lo_f, hi_f, stream=sptr)

        def find():
            b.find(d_text, n, d_sa, d_pat, nq * m, d_poff, nq, lo_s, hi_s, stream=sptr)

        fm_count()
        find()
        torch.cuda.synchronize()
        assert torch.equal(lo_f, lo_s) and torch.equal(hi_f, hi_s), f"intervals differ at {m} bytes"
        r = timed_events(torch, {"fm_count": fm_count, "find": find}, a.runs, a.warmup)
        for v in r.values():
            v["patterns_per_s"] = nq / (v["ms_median"] * 1e-3)
        r["pattern_bytes"] = m
        r["occurrences"] = int((u32(torch, hi_f) - u32(torch, lo_f)).sum())
        r["fm_count_over_find_median"] = r["fm_count"]["ms_median"] / r["find"]["ms_median"]
        out["count"].append(r)
        if m == LENGTHS[0]:
            keep = (lo_f, hi_f)
    d_lo, d_hi = keep
    d_off = torch.empty(nq + 1, dtype=torch.int64, device=dev)
    d_off2 = torch.empty(nq + 1, dtype=torch.int64, device=dev)
    total = b.fm_locate(d_index, ib, d_lo, d_hi, nq, d_off, None, 0, stream=sptr)
    d_pos = torch.full((total,), -1, dtype=torch.int32, device=dev)
    d_pos2 = torch.full((total,), -1, dtype=torch.int32, device=dev)

    def fm_locate():
        b.fm_locate(d_index, ib, d_lo, d_hi, nq, d_off, d_pos, total, stream=sptr)

    def locate():
        b.locate(n, d_sa, d_lo, d_hi, nq, d_off2, d_pos2, total, stream=sptr)

    fm_locate()
    locate()
    torch.cuda.synchronize()
    assert torch.equal(d_off, d_off2) and torch.equal(d_pos, d_pos2), "positions differ"
    r = timed_host(torch, {"fm_locate": fm_locate, "locate": locate}, a.runs, a.warmup)
    for v in r.values():
        v["ns_per_hit_median"] = v["ms_median"] * 1e6 / max(total, 1)
    r["hits"] = total
    r["pattern_bytes"] = LENGTHS[0]
    r["fm_locate_over_locate_median"] = r["fm_locate"]["ms_median"] / r["locate"]["ms_median"]
    out["locate"] = r
    b.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
