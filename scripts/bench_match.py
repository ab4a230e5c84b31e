#!/usr/bin/env python3
"""Throughput of the longest-match search (sa_match_device,
sa_matching_stats_device) on one MI355X, next to sa_find_device.

Generates a DNA text on the device and builds its suffix array with
DeviceBuilder.  Then

(a) batch form: for each pattern length it draws the batch bench_find.py
    draws (half cut from the text, half random, shuffled) and times
    sa_find_device, sa_match_device and sa_match_device without the bounds on
    it, in auto mode, and the first two on the text-sampled half alone: those
    patterns occur whole, both searches make the same probes, and the ratio
    of the two times is the cost of the match kernels themselves;
(b) sliding form: the query is a slice of the text with a substitution about
    every 50 bytes; the lane and the wave kernel are timed separately for
    max_len 32, 256 and 0 (none), each with and without the bounds.  Last,
    the two kernels on a slice of the text as it is, without a cap: position
    i matches everything that follows it, the case the lane kernel is not for.

Timing: every call is warmed up, then timed with device events in --rounds
windows of enough repetitions to fill --min-seconds together; the calls that
are compared alternate window by window.  Reported per call: the minimum and
the median window, as ns per query.  A few hundred batch results per length
are checked on the host from the gathered suffixes at lo - 1, lo, hi - 1 and
hi; the sliding form's kernels are checked against each other.  Prints one
JSON line.  There is no CPU path: with no GPU the script fails.

    python scripts/bench_match.py [--n 268435456] [--nq 1048576] [--query 1048576]
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

from scripts.bench_find import LENGTHS, MAX_PAT_BYTES, gather_windows   # noqa: E402

MAX_LENS = [32, 256, 0]


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 28)
    ap.add_argument("--nq", type=int, default=1 << 20)
    ap.add_argument("--query", type=int, default=1 << 20, help="bytes of the sliding form's query")
    ap.add_argument("--exact-query", type=int, default=1 << 16, help="bytes of the unchanged text slice")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--lengths", type=int, nargs="+", default=LENGTHS)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--spot", type=int, default=300, help="batch results checked on the host per length")
    return ap.parse_args()


def timed(torch, fns, nq, min_seconds, rounds):
    """{name: {ns_per_query_min, ns_per_query_median, reps}} of the calls in
    fns, alternating them window by window."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(fn, reps):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / reps

    reps = {}
    for name, fn in fns.items():
        fn()                                     # warm-up
        one = max(window(fn, 1), 1e-6)
        reps[name] = max(1, int(np.ceil(min_seconds / rounds / one)))
    secs = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            secs[name].append(window(fn, reps[name]))
    return {name: {"ns_per_query_min": min(s) / nq * 1e9, "ns_per_query_median": float(np.median(s)) / nq * 1e9,
                   "reps": reps[name], "rounds": rounds} for name, s in secs.items()}


def spot_check(torch, d_text, d_sa, pats, d_len, d_lo, d_hi, count, seed):
    """Host check of `count` results: the suffixes at lo and hi - 1 share
    exactly len bytes with the pattern (all of it when len == m), those at
    lo - 1 and hi fewer.  The pattern's insertion point lies in [lo, hi], so
    no suffix shares more than len."""
    n, (nq, m) = d_text.numel(), pats.shape
    g = torch.Generator(device="cpu").manual_seed(seed)
    pick = torch.randperm(nq, generator=g)[:count].to(d_text.device)
    u = lambda d: (d[pick].to(torch.int64) & 0xFFFFFFFF)   # noqa: E731
    ln, lo, hi = u(d_len).cpu().numpy(), u(d_lo), u(d_hi)
    p_host = pats[pick].cpu().numpy()
    rows = {}
    for name, r in (("lo-1", lo - 1), ("lo", lo), ("hi-1", hi - 1), ("hi", hi)):
        s = d_sa[r.clamp(0, n - 1)].to(torch.int64) & 0xFFFFFFFF
        rows[name] = (r.cpu().numpy(), s.cpu().numpy(), gather_windows(torch, d_text, s, m).cpu().numpy())

    def shared(name, i):
        r, s, w = rows[name]
        if r[i] < 0 or r[i] >= n:
            return -1
        lim = min(m, n - int(s[i]))
        diff = np.flatnonzero(w[i][:lim] != p_host[i][:lim])
        return int(diff[0]) if diff.size else lim
    for i in range(pick.numel()):
        assert 0 < ln[i] <= m, ("a DNA pattern matches at least one byte", i, ln[i])
        assert shared("lo", i) == ln[i] and shared("hi-1", i) == ln[i], ("not the match", i, ln[i])
        assert shared("lo-1", i) < ln[i] and shared("hi", i) < ln[i], ("interval too small", i, ln[i])
    return int(pick.numel())


def main():
    a = parse()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_match.py needs an MI355X: no HIP device is visible")
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
    out = {"bench": "match", "n": n, "kind": "dna", "seed": a.seed, "build_ms": st["total_ms"],
           "lane_max": N.FIND_LANE_MAX, "src_hash": N.source_hash(), "min_seconds": a.min_seconds,
           "rounds": a.rounds, "batch": {}, "sliding": {}}
    checked = 0
    for m in a.lengths:
        nq = max(2, min(a.nq, MAX_PAT_BYTES // m)) & ~1
        half = nq // 2
        pos = torch.randint(0, max(1, n - m + 1), (half,), generator=g, device=dev)
        cut = gather_windows(torch, d_text, pos, m)
        rnd = acgt[torch.randint(0, 4, (half, m), generator=g, device=dev)]
        mixed = torch.cat([cut, rnd])[torch.randperm(nq, generator=g, device=dev)].contiguous()
        d_off = (torch.arange(nq + 1, device=dev, dtype=torch.int64) * m)
        d_len, d_lo, d_hi, d_flo, d_fhi, d_len2 = (torch.empty(nq, dtype=torch.int32, device=dev) for _ in range(6))

        def calls(pats, q):
            return {"find": lambda: b.find(d_text, n, d_sa, pats, q * m, d_off, q, d_flo, d_fhi, stream=sptr),
                    "match": lambda: b.match(d_text, n, d_sa, pats, q * m, d_off, q, d_len, d_lo, d_hi, stream=sptr),
                    "match_lengths_only": lambda: b.match(d_text, n, d_sa, pats, q * m, d_off, q, d_len2, stream=sptr)}
        rec = {"nq": nq, "mixed": timed(torch, calls(mixed, nq), nq, a.min_seconds, a.rounds)}
        checked += spot_check(torch, d_text, d_sa, mixed, d_len, d_lo, d_hi, a.spot, a.seed + m)
        assert torch.equal(d_len, d_len2), "lengths-only differs"
        whole = (d_len.to(torch.int64) & 0xFFFFFFFF) == m
        assert torch.equal(d_lo[whole], d_flo[whole]) and torch.equal(d_hi[whole], d_fhi[whole]), "differs from find"
        assert bool((d_fhi[~whole] == d_flo[~whole]).all()), "find found a pattern that match did not"
        rec["whole_in_mixed"] = int(whole.sum())
        given = calls(cut, half)
        del given["match_lengths_only"]
        rec["text_given"] = timed(torch, given, half, a.min_seconds, a.rounds)
        assert bool(((d_len[:half].to(torch.int64) & 0xFFFFFFFF) == m).all()), "a pattern cut from the text did not match whole"
        for k in ("mixed", "text_given"):
            rec[k]["match_over_find_min"] = rec[k]["match"]["ns_per_query_min"] / rec[k]["find"]["ns_per_query_min"]
            rec[k]["match_over_find_median"] = (rec[k]["match"]["ns_per_query_median"]
                                                / rec[k]["find"]["ns_per_query_median"])
        out["batch"][str(m)] = rec
        del cut, rnd, mixed
    out["spot_checked"] = checked

    # sliding form: a slice of the text with a substitution about every 50 bytes
    mq = min(a.query, n)
    start = int(torch.randint(0, n - mq + 1, (1,), generator=g, device=dev))
    query = d_text[start:start + mq].clone()
    gaps = torch.randint(40, 61, (mq // 40 + 1,), generator=g, device=dev)
    at = torch.cumsum(gaps, 0)
    at = at[at < mq]
    other = torch.zeros(256, dtype=torch.uint8, device=dev)                 # another letter than the one given
    other[acgt.long()] = acgt.roll(1)
    query[at] = other[query[at].long()]
    d_len, d_lo, d_hi, d_len2 = (torch.empty(mq, dtype=torch.int32, device=dev) for _ in range(4))
    out["sliding"] = {"m": mq, "substitutions": int(at.numel()), "runs": {}}
    for max_len in MAX_LENS:
        fns, results = {}, {}
        for mode in ("lane", "wave"):
            fns[f"{mode}"] = (lambda mode=mode: b.matching_statistics(d_text, n, d_sa, query, mq, d_len, d_lo, d_hi,
                                                                      max_len=max_len, stream=sptr, mode=mode))
            fns[f"{mode}_lengths_only"] = (lambda mode=mode: b.matching_statistics(d_text, n, d_sa, query, mq, d_len2,
                                                                                   max_len=max_len, stream=sptr,
                                                                                   mode=mode))
        rec = timed(torch, fns, mq, a.min_seconds, a.rounds)
        for name, fn in fns.items():             # the four calls agree
            fn()
            torch.cuda.synchronize()
            results[name] = (d_len2 if name.endswith("only") else d_len).clone()
            if not name.endswith("only"):
                results[name + "/lo"], results[name + "/hi"] = d_lo.clone(), d_hi.clone()
        assert torch.equal(results["lane"], results["wave"]) and torch.equal(results["lane/lo"], results["wave/lo"])
        assert torch.equal(results["lane/hi"], results["wave/hi"])
        assert torch.equal(results["lane"], results["lane_lengths_only"])
        assert torch.equal(results["lane"], results["wave_lengths_only"])
        ln = results["lane"].to(torch.int64) & 0xFFFFFFFF
        rec["mean_len"], rec["max_len_found"] = float(ln.double().mean()), int(ln.max())
        out["sliding"]["runs"][str(max_len)] = rec
    # the other end: a slice of the text as it is, no cap.  Position i matches all m - i bytes that follow it, so
    # a lane's work grows with the query's length: what the auto rule's wave kernel is for
    me = min(a.exact_query, mq)
    exact = d_text[start:start + me].clone()
    fns = {mode: (lambda mode=mode: b.matching_statistics(d_text, n, d_sa, exact, me, d_len[:me] if mode == "lane"
                                                          else d_len2[:me], stream=sptr, mode=mode))
           for mode in ("lane", "wave")}
    rec = timed(torch, fns, me, a.min_seconds, a.rounds)
    want = torch.arange(me, 0, -1, device=dev, dtype=torch.int32)
    assert torch.equal(d_len[:me], want) and torch.equal(d_len2[:me], want), "a text slice matches to its end"
    out["sliding"]["exact"] = dict(rec, m=me)
    b.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
