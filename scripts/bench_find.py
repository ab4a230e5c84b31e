#!/usr/bin/env python3
"""Throughput of the batched pattern search (sa_find_device) on one MI355X.

Generates a DNA text on the device, builds its suffix array with
DeviceBuilder, and for each pattern length draws a batch from the seed -- half
cut from the text, half random, shuffled -- and times sa_find_device with
device events after a warm-up, over enough repetitions to fill at least
--min-seconds.  Per length it reports queries/s and ns/query for the three
modes (lane, wave, auto) and, for the text-sampled half alone, in the drawn
order and sorted by pattern (neighbouring lanes then descend together).
A few hundred results are checked on the host from the gathered SA[lo - 1],
SA[lo], SA[hi - 1], SA[hi].  Prints one JSON line.  There is no CPU path: with
no GPU the script fails.

    python scripts/bench_find.py [--n 268435456] [--nq 1048576]
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

LENGTHS = [12, 32, 128, 1024, 16384]
MODES = ["lane", "wave", "auto"]
MAX_PAT_BYTES = 1 << 30     # a batch of long patterns is cut to this many bytes


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 28)
    ap.add_argument("--nq", type=int, default=1 << 20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--lengths", type=int, nargs="+", default=LENGTHS)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--spot", type=int, default=300, help="results checked on the host per length")
    return ap.parse_args()


def gather_windows(torch, d_text, pos, m):
    """(len(pos), m) bytes of the text at pos (clipped to the text's end), in pieces."""
    n = d_text.numel()
    out = torch.empty((pos.numel(), m), dtype=torch.uint8, device=d_text.device)
    ar = torch.arange(m, device=d_text.device)
    step = max(1, (1 << 25) // m)
    for a in range(0, pos.numel(), step):
        idx = pos[a:a + step, None] + ar[None, :]
        out[a:a + step] = d_text[idx.clamp_(max=n - 1)]
    return out


def timed(torch, fn, min_seconds):
    fn()                                     # warm-up
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    one = max(e0.elapsed_time(e1) * 1e-3, 1e-6)
    reps = max(1, int(np.ceil(min_seconds / one)))
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps, reps


def spot_check(torch, d_text, d_sa, pats, d_lo, d_hi, count, seed):
    """Host check of `count` results: the suffixes at lo and hi - 1 start with
    the pattern, the one at lo - 1 is below it and the one at hi above it."""
    n, (nq, m) = d_text.numel(), pats.shape
    g = torch.Generator(device="cpu").manual_seed(seed)
    pick = torch.randperm(nq, generator=g)[:count].to(d_text.device)
    lo = (d_lo[pick].to(torch.int64) & 0xFFFFFFFF)
    hi = (d_hi[pick].to(torch.int64) & 0xFFFFFFFF)
    sa64 = lambda r: d_sa[r.clamp(0, n - 1)].to(torch.int64) & 0xFFFFFFFF   # noqa: E731
    rows = {}
    for name, r in (("lo-1", lo - 1), ("lo", lo), ("hi-1", hi - 1), ("hi", hi)):
        s = sa64(r)
        rows[name] = (r.cpu().numpy(), s.cpu().numpy(), gather_windows(torch, d_text, s, m).cpu().numpy())
    p_host = pats[pick].cpu().numpy()
    lo_h, hi_h = lo.cpu().numpy(), hi.cpu().numpy()
    for i in range(pick.numel()):
        p = p_host[i].tobytes()

        def suffix(name):
            r, s, w = rows[name]
            return None if r[i] < 0 or r[i] >= n else w[i].tobytes()[:min(m, n - int(s[i]))]
        assert lo_h[i] <= hi_h[i] <= n, (lo_h[i], hi_h[i])
        below, first, last, above = suffix("lo-1"), suffix("lo"), suffix("hi-1"), suffix("hi")
        if hi_h[i] > lo_h[i]:
            assert first == p and last == p, ("not a match", i, lo_h[i], hi_h[i])
        assert below is None or below < p, ("lo too high", i, lo_h[i])
        assert above is None or (above > p and not above.startswith(p)), ("hi too low", i, hi_h[i])
    return int(pick.numel())


def main():
    a = parse()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_find.py needs an MI355X: no HIP device is visible")
    from hpc_suffix_array_amd import DeviceBuilder, _native as N
    dev = torch.device("cuda", 0)
    n = a.n
    b = DeviceBuilder(n)
    d_text = torch.empty(n, dtype=torch.uint8, device=dev)
    b.generate_text(d_text, n, b"ACGT", seed=a.seed)
    d_sa = torch.empty(n, dtype=torch.int32, device=dev)
    st = b.build(d_text, n, d_sa)
    torch.cuda.synchronize()
    sptr = torch.cuda.current_stream(dev).cuda_stream
    g = torch.Generator(device=dev).manual_seed(a.seed)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    out = {"bench": "find", "n": n, "kind": "dna", "seed": a.seed, "build_ms": st["total_ms"],
           "lane_max": N.FIND_LANE_MAX, "src_hash": N.source_hash(), "min_seconds": a.min_seconds, "lengths": {}}
    checked = 0
    for m in a.lengths:
        nq = max(2, min(a.nq, MAX_PAT_BYTES // m)) & ~1
        half = nq // 2
        pos = torch.randint(0, max(1, n - m + 1), (half,), generator=g, device=dev)
        cut = gather_windows(torch, d_text, pos, m)
        rnd = acgt[torch.randint(0, 4, (half, m), generator=g, device=dev)]
        mixed = torch.cat([cut, rnd])[torch.randperm(nq, generator=g, device=dev)].contiguous()
        d_off = (torch.arange(nq + 1, device=dev, dtype=torch.int64) * m)
        d_lo = torch.empty(nq, dtype=torch.int32, device=dev)
        d_hi = torch.empty(nq, dtype=torch.int32, device=dev)
        rec = {"nq": nq}

        def run(pats, q, mode):
            return lambda: b.find(d_text, n, d_sa, pats, q * m, d_off, q, d_lo, d_hi, stream=sptr, mode=mode)
        for mode in MODES:
            sec, reps = timed(torch, run(mixed, nq, mode), a.min_seconds)
            rec[mode] = {"queries_per_s": nq / sec, "ns_per_query": sec / nq * 1e9, "reps": reps}
        checked += spot_check(torch, d_text, d_sa, mixed, d_lo, d_hi, a.spot, a.seed + m)   # the auto run's results
        # the text-sampled half alone: drawn order, then sorted by pattern (= by lo)
        sec, reps = timed(torch, run(cut, half, "auto"), a.min_seconds)
        rec["text_given"] = {"queries_per_s": half / sec, "ns_per_query": sec / half * 1e9, "reps": reps}
        order = torch.argsort(d_lo[:half].to(torch.int64) & 0xFFFFFFFF)
        cut_sorted = cut[order].contiguous()
        sec, reps = timed(torch, run(cut_sorted, half, "auto"), a.min_seconds)
        rec["text_sorted"] = {"queries_per_s": half / sec, "ns_per_query": sec / half * 1e9, "reps": reps}
        assert bool((d_hi[:half] != d_lo[:half]).all()), "a pattern cut from the text was not found"
        out["lengths"][str(m)] = rec
        del cut, rnd, mixed, cut_sorted
    out["spot_checked"] = checked
    b.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
