#!/usr/bin/env python3
"""Time of the Burrows-Wheeler transform and the inverse suffix array of a
built SA (sa_bwt_device, sa_inverse_device) on one MI355X, next to the only
way to get the BWT on the GPU without them: the torch indexing expression
``text[(sa.to(torch.int64) - 1) % n]``.

For each text kind (random DNA, random bytes over all 256 values) and each n
it generates the text on the device, builds its suffix array in place with
DeviceBuilder and times, on the same GPU,

    bwt           sa_bwt_device without statistics
    bwt_stats     sa_bwt_device with primary index, runs and histogram
    inverse       sa_inverse_device (it waits for the stream itself)
    torch_index   text[(sa.to(torch.int64) - 1) % n]

Timing: every call is warmed up, then timed alone between two device events,
--runs times (at least 20), the four calls alternating run by run; reported
per call: the median and the minimum in ms.  The outputs are checked against
each other first: the kernel's bytes equal the torch expression's, the
histogram equals torch.bincount of the text, the primary index equals ISA[0],
and ISA[SA[r]] = r on a sample.  Prints one JSON line.  There is no CPU path:
with no GPU the script fails.

    python scripts/bench_bwt.py [--n 268435456 1073741824] [--kinds dna byte256] [--runs 20]
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

ALPHABETS = {"dna": b"ACGT", "byte256": bytes(range(256))}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1 << 28, 1 << 30])
    ap.add_argument("--kinds", nargs="+", default=["dna", "byte256"], choices=sorted(ALPHABETS))
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    return ap.parse_args()


def timed(torch, fns, runs, warmup):
    """{name: {ms_median, ms_min, runs}}: one call per window, the calls
    alternating run by run."""
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
    return {name: {"ms_median": float(np.median(v)), "ms_min": min(v), "runs": runs} for name, v in ms.items()}


def one(torch, a, kind, n):
    from hpc_suffix_array_amd import DeviceBuilder, _native as N
    dev = torch.device("cuda", 0)
    b = DeviceBuilder(n)
    d_text = torch.empty(n, dtype=torch.uint8, device=dev)
    b.generate_text(d_text, n, ALPHABETS[kind], seed=a.seed)
    d_sa = torch.empty(n, dtype=torch.int32, device=dev)
    st = b.build(d_text, n, d_sa)
    d_bwt = torch.empty(n, dtype=torch.uint8, device=dev)
    d_bwt2 = torch.empty(n, dtype=torch.uint8, device=dev)
    d_stats = torch.empty(N.BWT_STATS, dtype=torch.int64, device=dev)
    d_isa = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    sptr = torch.cuda.current_stream(dev).cuda_stream
    # (the expression as a user writes it; an int32 tensor holds positions up to 2^31 - 1)
    assert n <= 1 << 31, "the torch expression reads the SA as int32"
    index = lambda: d_text[(d_sa.to(torch.int64) - 1) % n]   # noqa: E731

    # the outputs agree before anything is timed
    b.bwt(d_text, n, d_sa, d_bwt, stream=sptr)
    b.bwt(d_text, n, d_sa, d_bwt2, d_stats, stream=sptr)
    b.inverse(n, d_sa, d_isa, stream=sptr)
    want = index()
    assert torch.equal(d_bwt, want) and torch.equal(d_bwt2, want), "BWT differs from the torch expression"
    stats = d_stats.cpu().numpy()
    assert (stats[2:] == torch.bincount(d_text, minlength=256).cpu().numpy()).all(), "histogram"
    assert int(stats[1]) == 1 + int((want[1:] != want[:-1]).sum()), "runs"
    assert int(stats[0]) == int(d_isa[0]) & 0xFFFFFFFF, "primary index"
    g = torch.Generator(device=dev).manual_seed(a.seed)
    r = torch.randint(0, n, (1 << 20,), generator=g, device=dev)
    assert torch.equal(d_isa[d_sa[r].to(torch.int64) & 0xFFFFFFFF].to(torch.int64) & 0xFFFFFFFF, r), "ISA[SA[r]] != r"
    del want, r

    def torch_index():
        index()

    fns = {"bwt": lambda: b.bwt(d_text, n, d_sa, d_bwt, stream=sptr),
           "bwt_stats": lambda: b.bwt(d_text, n, d_sa, d_bwt2, d_stats, stream=sptr),
           "inverse": lambda: b.inverse(n, d_sa, d_isa, stream=sptr),
           "torch_index": torch_index}
    rec = timed(torch, fns, max(20, a.runs), a.warmup)
    rec.update(kind=kind, n=n, build_ms=st["total_ms"], primary=int(stats[0]), runs_in_bwt=int(stats[1]),
               bwt_over_torch_median=rec["bwt"]["ms_median"] / rec["torch_index"]["ms_median"],
               stats_extra_ms_median=rec["bwt_stats"]["ms_median"] - rec["bwt"]["ms_median"],
               bwt_ns_per_rank_median=rec["bwt"]["ms_median"] * 1e6 / n)
    b.close()
    del d_text, d_sa, d_bwt, d_bwt2, d_isa
    torch.cuda.empty_cache()
    return rec


def main():
    a = parse()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_bwt.py needs an MI355X: no HIP device is visible")
    from hpc_suffix_array_amd import _native as N
    out = {"bench": "bwt", "seed": a.seed, "tile": N.BWT_TILE, "src_hash": N.source_hash(),
           "cus": torch.cuda.get_device_properties(0).multi_processor_count, "results": []}
    for kind in a.kinds:
        for n in a.n:
            out["results"].append(one(torch, a, kind, n))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
