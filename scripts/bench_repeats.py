#!/usr/bin/env python3
"""Time of the repeat enumeration over a built SA (sa_repeats_device) on one
MI355X, next to sa_lpf_device with the LCP given in the same process as the
yardstick: the same hierarchy and walk shape, but it resolves every rank and
scatters 8 bytes per rank.

For each case (random DNA at the large sizes; at 2^24 also a^(n-1)b, one
symbol and the Fibonacci word, whose LCP arrays are the walks' worst cases) it
puts the text on the device, builds its suffix array and its LCP array with
DeviceBuilder and times, all with d_lcp given,

    right_size / right_write       SA_REP_RIGHT, min_len 1: the sizing call
                                   (NULL outputs) and the writing call
    maximal_size / maximal_write   SA_REP_MAXIMAL, min_len 1
    super_size / super_write       SA_REP_SUPERMAXIMAL, min_len 1
    maximal20_size / maximal20_write   SA_REP_MAXIMAL, min_len 20
    lpf                            sa_lpf_device (enqueue only; the window
                                   ends in a device event)

Timing: every call is warmed up, then timed alone between two device events,
--runs times, the calls alternating run by run; reported per call: the median,
the minimum and the maximum in ms, and the ratios of the medians to lpf's.
The outputs are checked first, on the device: every interval is closed by
smaller LCP entries on both sides and holds none below its length at its
edges, its first and last suffix agree on the first and the last byte of the
repeat and differ behind it; the sizing and the writing call agree; the kinds
are nested; a right-maximal repeat is listed as maximal exactly when the
symbols in front of its occurrences change somewhere (a running count of
changes by a torch expression); a supermaximal one has at most 257
occurrences.  Prints one JSON line and writes it to --out.  There is no CPU
path: with no GPU the script fails.

    python scripts/bench_repeats.py [--n 268435456] [--adversarial-n 16777216] [--runs 10]
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

CONFIGS = {"right": ("right", 1), "maximal": ("maximal", 1), "super": ("supermaximal", 1), "maximal20": ("maximal", 20)}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[1 << 28])
    ap.add_argument("--adversarial-n", type=int, nargs="*", default=[1 << 24])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_repeats.json"))
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


def u32(x):
    """An int32 tensor's values as the uint32 they are, in int64."""
    import torch
    return x.to(torch.int64) & 0xFFFFFFFF


def fibonacci(n):
    a, b = b"a", b"ab"
    while len(b) < n:
        a, b = b, b + a
    return b[:n]


def check_intervals(torch, n, d_text, d_sa, d_lcp, ln, lo, hi):
    """What every listed repeat must satisfy, on the device."""
    if ln.numel() == 0:
        return
    L, A, B = u32(ln), u32(lo), u32(hi)
    lcp, sa = u32(d_lcp), u32(d_sa)
    lcp[0] = 0
    assert bool((L >= 1).all()) and bool((B - A >= 2).all()) and bool((B <= n).all()), "len >= 1, two occurrences"
    assert bool((lcp[A] < L).all()), "lcp[lo] < len"
    inner = B < n
    assert bool((lcp[B[inner]] < L[inner]).all()), "lcp[hi] < len"
    assert bool((lcp[A + 1] >= L).all()) and bool((lcp[B - 1] >= L).all()), "lcp >= len at the edges inside"
    p, q = sa[A], sa[B - 1]                         # the first and the last suffix of the interval
    assert bool((p + L <= n).all()) and bool((q + L <= n).all()), "the repeat inside the text"
    assert bool((d_text[p] == d_text[q]).all()) and bool((d_text[p + L - 1] == d_text[q + L - 1]).all()), "one string"
    both = (p + L < n) & (q + L < n)
    assert bool((d_text[(p + L)[both]] != d_text[(q + L)[both]]).all()), "right-maximal"
    key = A * (n + 1) + B
    assert bool((key[1:] != key[:-1]).all()), "an interval is listed once"


def one(torch, a, kind, n):
    from hpc_suffix_array_amd import DeviceBuilder
    dev = torch.device("cuda", 0)
    b = DeviceBuilder(n)
    if kind == "dna":
        d_text = torch.empty(n, dtype=torch.uint8, device=dev)
        b.generate_text(d_text, n, b"ACGT", seed=a.seed)
    elif kind == "fibonacci":
        d_text = torch.from_numpy(np.frombuffer(fibonacci(n), np.uint8).copy()).to(dev)
    else:
        d_text = torch.full((n,), ord("a"), dtype=torch.uint8, device=dev)
        if kind == "a_b":
            d_text[-1] = ord("b")
    d_sa = torch.empty(n, dtype=torch.int32, device=dev)
    st = b.build(d_text, n, d_sa)
    d_lcp, d_lpf, d_src = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    torch.cuda.synchronize()
    sptr = torch.cuda.current_stream(dev).cuda_stream
    b.lcp(d_text, n, d_sa, d_lcp, stream=sptr)

    # the outputs are checked before anything is timed
    outs, counts = {}, {}
    for name, (k, min_len) in CONFIGS.items():
        count, occ = b.repeats(d_text, n, d_sa, d_lcp, min_len, 2, k, None, None, None, 0, stream=sptr)
        o = tuple(torch.empty(max(count, 1), dtype=torch.int32, device=dev) for _ in range(3))
        assert b.repeats(d_text, n, d_sa, d_lcp, min_len, 2, k, *o, count, stream=sptr) == (count, occ), "sizing != writing"
        o = tuple(x[:count] for x in o)
        check_intervals(torch, n, d_text, d_sa, d_lcp, *o)
        assert int((u32(o[2]) - u32(o[1])).sum()) == occ, "info[1] is the sum of hi - lo"
        outs[name], counts[name] = o, {"count": count, "total_occ": occ}
    # the kinds are nested, and maximal is right-maximal with a change of the preceding symbol inside
    s = u32(d_sa)
    prev = torch.where(s > 0, d_text[torch.clamp(s, min=1) - 1].to(torch.int64), 256)
    del s
    changes = torch.zeros(n, dtype=torch.int64, device=dev)
    changes[1:] = torch.cumsum(prev[1:] != prev[:-1], 0)
    del prev
    keys = {name: u32(o[1]) * (n + 1) + u32(o[2]) for name, o in outs.items()}
    if counts["right"]["count"]:
        lo, hi = u32(outs["right"][1]), u32(outs["right"][2])
        left_max = changes[hi - 1] != changes[lo]
        assert torch.equal(keys["right"][left_max], keys["maximal"]), "maximal = right-maximal and left-maximal"
        assert bool(torch.isin(keys["super"], keys["maximal"]).all()), "supermaximal within maximal"
        assert bool((u32(outs["super"][2]) - u32(outs["super"][1]) <= 257).all()), "at most 257 occurrences"
        long = u32(outs["maximal"][0]) >= 20
        assert torch.equal(keys["maximal"][long], keys["maximal20"]), "min_len filters"
        del lo, hi, left_max, long
    del changes, keys
    torch.cuda.empty_cache()

    fns = {}
    for name, (k, min_len) in CONFIGS.items():
        o, count = outs[name], counts[name]["count"]
        fns[name + "_size"] = (lambda k=k, m=min_len: b.repeats(d_text, n, d_sa, d_lcp, m, 2, k, None, None, None, 0,
                                                                 stream=sptr))
        fns[name + "_write"] = (lambda k=k, m=min_len, o=o, c=count: b.repeats(d_text, n, d_sa, d_lcp, m, 2, k,
                                                                               o[0], o[1], o[2], c, stream=sptr))
    fns["lpf"] = lambda: b.lpf(None, n, d_sa, d_lcp, d_lpf, d_src, stream=sptr)
    rec = timed(torch, fns, a.runs, a.warmup)
    lpf = rec["lpf"]["ms_median"]
    rec.update(kind=kind, n=n, build_ms=st["total_ms"], counts=counts,
               over_lpf_median={name: rec[name]["ms_median"] / lpf for name in fns if name != "lpf"},
               maximal_write_ns_per_rank_median=rec["maximal_write"]["ms_median"] * 1e6 / n)
    b.close()
    del outs, d_text, d_sa, d_lcp, d_lpf, d_src
    torch.cuda.empty_cache()
    return rec


def main():
    a = parse()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_repeats.py needs an MI355X: no HIP device is visible")
    from hpc_suffix_array_amd import _native as N
    out = {"bench": "repeats", "seed": a.seed, "tile": N.LZ_TILE, "src_hash": N.source_hash(),
           "cus": torch.cuda.get_device_properties(0).multi_processor_count, "results": []}
    for n in a.n:
        out["results"].append(one(torch, a, "dna", n))
    for n in a.adversarial_n:
        dna = one(torch, a, "dna", n)
        out["results"].append(dna)
        for kind in ("a_b", "one", "fibonacci"):
            rec = one(torch, a, kind, n)
            # the bounded-walk claim: a worst-case LCP array against random text of the same length
            rec["over_dna_median"] = {name: rec[name]["ms_median"] / dna[name]["ms_median"]
                                      for name in rec if isinstance(rec[name], dict) and "ms_median" in rec[name]}
            out["results"].append(rec)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
