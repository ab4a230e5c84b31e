#!/usr/bin/env python3
"""Time of the LCE entry points (sa_lce_build_device, sa_lcp_min_device,
sa_lce_device) on one MI355X, next to what a device caller writes without
them in plain torch on the same GPU:

    build     torch.amin over the (n / 64, 64) view of LCP: one streaming
              reduction of the same array, the cost of reading LCP once
    queries   a full sparse table (torch.minimum of shifted views, log2 n
              levels of n words) plus two gathers and a minimum per query;
              built only up to --table-max bytes of table

Those torch expressions are the baseline, not the code under test.

Texts, generated on the device from a seed: random DNA, and "repeat": random
DNA whose second half copies the first with one substitution every --period
bytes, so every suffix of one half shares up to --period bytes with its twin.
The suffix array, LCP and ISA are built in place with the library.  Query
batches: random position pairs (on random DNA nearly all differ in the first
bytes), "twin" pairs (i, i + n / 2) of the repeat text (long extensions), and
random rank intervals.  The position forms run with and without the text
probe; the outputs of both, and of the torch table where it is built, are
compared before anything is timed.  Each measurement is warmed up, then a
window of --reps calls is timed between two device events, --runs times.
Reported: median, minimum and maximum ms per call and ns per query.  Prints one
JSON line and writes it to --out when given.  With no GPU the script fails.

    python scripts/bench_lce.py [--n 16777216 268435456] [--nq 1048576 16777216] [--runs 10] [--out profiles/bench_lce.json]
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


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1 << 24, 1 << 28])
    ap.add_argument("--nq", type=int, nargs="+", default=[1 << 20, 1 << 24])
    ap.add_argument("--texts", nargs="+", default=["dna", "repeat"], choices=["dna", "repeat"])
    ap.add_argument("--period", type=int, default=4096)
    ap.add_argument("--table-max", type=int, default=4 << 30, help="largest torch sparse table built, in bytes")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--reps", type=int, default=0, help="calls per timed window (0: 2^25 / nq, at least 1)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    return ap.parse_args()


def timed(torch, fn, runs, warmup, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return {"ms_median": float(np.median(ms)), "ms_min": min(ms), "ms_max": max(ms), "runs": runs, "reps": reps}


def per_query(res, nq):
    res["ns_per_query"] = res["ms_median"] * 1e6 / nq
    return res


def make_text(torch, b, kind, n, seed, period):
    d_text = torch.zeros(n + 256, dtype=torch.uint8, device="cuda")[:n]
    b.generate_text(d_text, n, b"ACGT", seed)
    if kind == "repeat":
        half = n // 2
        d_text[half:2 * half] = d_text[:half]
        at = torch.arange(half + period // 2, 2 * half, period, device="cuda")
        d_text[at] = torch.where(d_text[at] == ord("A"), ord("C"), ord("A")).to(torch.uint8)
    return d_text


def torch_table(torch, lcp):
    """Level k holds min lcp[r .. r + 2^k): log2 n levels of n words."""
    levels = [lcp]
    n, k = lcp.numel(), 1
    while (1 << k) <= n:
        prev, half = levels[-1], 1 << (k - 1)
        cur = prev.clone()
        cur[:n - half] = torch.minimum(prev[:n - half], prev[half:])
        levels.append(cur)
        k += 1
    return torch.stack(levels)


def torch_range_min(torch, table, x, y):
    """min lcp[x .. y] (inclusive, int64 tensors, x <= y) by two gathers."""
    ln = y - x + 1
    one = torch.ones_like(ln)
    k = torch.log2(ln.to(torch.float64)).floor().to(torch.int64)   # floor(log2 ln), mended where the float rounds
    k = torch.where(torch.bitwise_left_shift(one, k + 1) <= ln, k + 1, k)
    k = torch.where(torch.bitwise_left_shift(one, k) > ln, k - 1, k)
    n = table.shape[1]
    flat = table.reshape(-1)
    return torch.minimum(flat[k * n + x], flat[k * n + y - torch.bitwise_left_shift(one, k) + 1])


def main():
    args = parse()
    import torch

    from hpc_suffix_array_amd import DeviceBuilder, _native as N
    if not torch.cuda.is_available() or N.device_count() <= 0:
        raise SystemExit("bench_lce.py needs an MI355X")
    out = {"bench": "lce", "device": torch.cuda.get_device_name(0), "source_hash": N.source_hash(), "period": args.period,
           "cases": []}
    for n in args.n:
        b = DeviceBuilder(n)
        for kind in args.texts:
            case = {"n": n, "text": kind}
            d_text = make_text(torch, b, kind, n, args.seed, args.period)
            d_sa = torch.zeros(n + 64, dtype=torch.int32, device="cuda")[:n]
            d_lcp = torch.zeros(n + 64, dtype=torch.int32, device="cuda")[:n]
            d_isa = torch.zeros(n + 64, dtype=torch.int32, device="cuda")[:n]
            st = b.build(d_text, n, d_sa)
            b.lcp(d_text, n, d_sa, d_lcp)
            b.inverse(n, d_sa, d_isa)
            del d_sa
            torch.cuda.synchronize()
            case["sa_build_ms"] = st["total_ms"]
            case["lcp_max"] = int(d_lcp.max().item())
            index = b.lce_build(d_lcp)
            case["index_bytes"] = int(index.numel())
            # the build next to one streaming reduction of the same array
            view = d_lcp[:n - n % 64].view(-1, 64)
            assert torch.equal(torch.amin(view, dim=1), index[4096:4096 + 4 * (n // 64)].view(torch.int32)), "block minima"
            reps = 4
            case["build"] = timed(torch, lambda: b.lce_build(d_lcp), args.runs, args.warmup, reps)
            case["torch_amin"] = timed(torch, lambda: torch.amin(view, dim=1), args.runs, args.warmup, reps)
            case["build"]["gb_per_s"] = 4 * n / case["build"]["ms_median"] / 1e6
            case["torch_amin"]["gb_per_s"] = 4 * n / case["torch_amin"]["ms_median"] / 1e6
            table = None
            levels = n.bit_length()
            case["torch_table_bytes"] = 4 * n * levels
            if case["torch_table_bytes"] <= args.table_max:
                case["torch_table_build"] = timed(torch, lambda: torch_table(torch, d_lcp), 3, 1, 1)
                table = torch_table(torch, d_lcp)
            case["queries"] = []
            for nq in args.nq:
                reps = args.reps or max(1, (1 << 25) // nq)
                g = torch.Generator(device="cuda")
                g.manual_seed(args.seed + nq)
                batches = {"random": (torch.randint(0, n, (nq,), generator=g, device="cuda", dtype=torch.int64),
                                      torch.randint(0, n, (nq,), generator=g, device="cuda", dtype=torch.int64))}
                if kind == "repeat":
                    i = torch.randint(0, n // 2, (nq,), generator=g, device="cuda", dtype=torch.int64)
                    batches["twin"] = (i, i + n // 2)
                for name, (i64, j64) in batches.items():
                    i, j = i64.to(torch.int32), j64.to(torch.int32)
                    plain = b.lce(d_isa, d_lcp, index, i, j)
                    probe = b.lce(d_isa, d_lcp, index, i, j, text=d_text)
                    assert torch.equal(plain, probe), "the probe changes an answer"
                    q = {"nq": nq, "batch": name, "form": "positions", "mean_lce": float(plain.double().mean().item()),
                         "answered_by_probe": float((plain < N.LCE_PROBE).double().mean().item())}
                    o = torch.empty(nq, dtype=torch.int32, device="cuda")
                    q["no_probe"] = per_query(timed(torch, lambda: b.lce(d_isa, d_lcp, index, i, j, out=o), args.runs,
                                                    args.warmup, reps), nq)
                    q["probe"] = per_query(timed(torch, lambda: b.lce(d_isa, d_lcp, index, i, j, text=d_text, out=o),
                                                 args.runs, args.warmup, reps), nq)
                    if table is not None:
                        def torch_lce():
                            ra, rb = d_isa[i64].to(torch.int64), d_isa[j64].to(torch.int64)
                            x, y = torch.minimum(ra, rb) + 1, torch.maximum(ra, rb)
                            same = x > y
                            return torch.where(same, n - i64, torch_range_min(torch, table, torch.where(same, y, x), y))
                        assert torch.equal(torch_lce().to(torch.int32), plain), "torch table against the kernel"
                        q["torch"] = per_query(timed(torch, torch_lce, 3, 1, 1), nq)
                    case["queries"].append(q)
                lo, hi = torch.sort(torch.randint(0, n + 1, (2, nq), generator=g, device="cuda", dtype=torch.int64), dim=0)[0]
                hi = torch.clamp(torch.maximum(hi, lo + 2), max=n)        # at least one rank under the minimum
                lo = torch.minimum(lo, hi - 2)
                lo32, hi32 = lo.to(torch.int32), hi.to(torch.int32)
                got = b.lcp_min(d_lcp, index, lo32, hi32)
                q = {"nq": nq, "batch": "random", "form": "rank intervals"}
                o = torch.empty(nq, dtype=torch.int32, device="cuda")
                q["kernel"] = per_query(timed(torch, lambda: b.lcp_min(d_lcp, index, lo32, hi32, out=o), args.runs, args.warmup,
                                              reps), nq)
                if table is not None:
                    assert torch.equal(torch_range_min(torch, table, lo + 1, hi - 1), got), "torch table against the kernel"
                    q["torch"] = per_query(timed(torch, lambda: torch_range_min(torch, table, lo + 1, hi - 1), 3, 1, 1), nq)
                case["queries"].append(q)
            del table
            out["cases"].append(case)
            print(json.dumps(case), file=sys.stderr, flush=True)
        b.close()
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
