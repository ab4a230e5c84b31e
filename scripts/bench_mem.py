#!/usr/bin/env python3
"""Time of the maximal exact matches (sa_mems_device) on one MI355X, next to
its two parts measured in the same process: the seed search
(sa_matching_stats_device with max_len = L) and the locate of the seeds' hits
(sa_locate_device on the same intervals).  There is no pass/fail number: what
comes after the seeds should cost the same order as locating those hits.

The text is random DNA (2^28 by default), generated on the device, its SA
built in place.  Workloads:

    subst    a 1 MiB query cut from the text with a substitution about every
             50 bytes; L = 16, 20, 32; max_occ = 0 and 64
    slice    a 64 KiB and a 1 MiB slice of the text as it is (one very long
             MEM among short ones), L = 20, under auto / lane / wave
    blocks   1 MiB queries made of blocks of B bytes cut from the text, a
             changed byte between them (every extension about B bytes long),
             under lane and wave: where the two cross is where a lane should
             hand over (kMemLaneBytes of csrc/sa_mem.h)

Each call is warmed up and timed alone between two device events, --runs
times, the calls of one workload alternating run by run.  Reported per call:
median, minimum and maximum in ms; ns per candidate and per MEM; the shares of
the seed search and of the locate.  Prints one JSON line and writes it to
--out when given.  With no GPU the script fails.

    python scripts/bench_mem.py [--n 268435456] [--runs 20] [--out profiles/bench_mem.json]
    python scripts/bench_mem.py --workloads subst --runs 3 --warmup 1     # a short run for a kernel trace
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
    ap.add_argument("--n", type=int, default=1 << 28)
    ap.add_argument("--m", type=int, default=1 << 20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workloads", nargs="+", default=["subst", "slice", "blocks"],
                    choices=["subst", "slice", "blocks"])
    ap.add_argument("--blocks", nargs="+", type=int, default=[64, 128, 256, 512, 1024, 2048, 4096, 16384])
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


class Bench:
    def __init__(self, torch, a, b, d_text, d_sa):
        self.torch, self.a, self.b, self.d_text, self.d_sa = torch, a, b, d_text, d_sa
        self.dev = d_text.device
        self.sptr = torch.cuda.current_stream(self.dev).cuda_stream

    def other_symbol(self, x):
        """Another symbol of ACGT for each byte of x (A -> C -> G -> T -> A)."""
        table = self.torch.zeros(256, dtype=self.torch.uint8, device=self.dev)
        for c, d in zip(b"ACGT", b"CGTA"):
            table[c] = d
        return table[x.to(self.torch.int64)]

    def sized(self, d_q, L, max_occ, mode):
        """(d_off, d_tpos, d_len, (total, candidates, skipped)) after the sizing call."""
        torch, m = self.torch, d_q.numel()
        d_off = torch.empty(m + 1, dtype=torch.int64, device=self.dev)
        info = self.b.mems(self.d_text, self.a.n, self.d_sa, d_q, m, L, d_off, None, None, 0, max_occ=max_occ,
                           mode=mode, stream=self.sptr)
        d_tpos = torch.empty(max(info[0], 1), dtype=torch.int32, device=self.dev)
        d_len = torch.empty(max(info[0], 1), dtype=torch.int32, device=self.dev)
        return d_off, d_tpos, d_len, info

    def mems_fn(self, d_q, L, max_occ, mode):
        d_off, d_tpos, d_len, info = self.sized(d_q, L, max_occ, mode)
        m = d_q.numel()

        def fn():
            self.b.mems(self.d_text, self.a.n, self.d_sa, d_q, m, L, d_off, d_tpos, d_len, info[0], max_occ=max_occ,
                        mode=mode, stream=self.sptr)
        return fn, info, (d_off, d_tpos, d_len)

    def parts(self, d_q, L, max_occ):
        """The seed search alone and the locate of the same intervals alone."""
        torch, m, n = self.torch, d_q.numel(), self.a.n
        d_l = torch.empty(m, dtype=torch.int32, device=self.dev)
        d_lo = torch.empty(m, dtype=torch.int32, device=self.dev)
        d_hi = torch.empty(m, dtype=torch.int32, device=self.dev)

        def seeds():
            self.b.matching_statistics(self.d_text, n, self.d_sa, d_q, m, d_l, d_lo, d_hi, max_len=L, stream=self.sptr)
        seeds()
        torch.cuda.synchronize()
        lo = d_lo.to(torch.int64) & 0xFFFFFFFF
        cnt = (d_hi.to(torch.int64) & 0xFFFFFFFF) - lo
        keep = (d_l.to(torch.int64) == L) & ((cnt <= max_occ) if max_occ else torch.ones_like(cnt, dtype=torch.bool))
        d_hi2 = torch.where(keep, lo + cnt, lo).to(torch.int32)
        d_off = torch.empty(m + 1, dtype=torch.int64, device=self.dev)
        total = self.b.locate(n, self.d_sa, d_lo, d_hi2, m, d_off, None, 0, stream=self.sptr)
        d_pos = torch.empty(max(total, 1), dtype=torch.int32, device=self.dev)

        def locate():
            self.b.locate(n, self.d_sa, d_lo, d_hi2, m, d_off, d_pos, total, stream=self.sptr)
        return seeds, locate, total

    def record(self, r, info):
        for v in r.values():
            v["ns_per_candidate"] = v["ms_median"] * 1e6 / max(info[1], 1)
            v["ns_per_mem"] = v["ms_median"] * 1e6 / max(info[0], 1)
        return r

    def subst(self):
        torch, a = self.torch, self.a
        g = torch.Generator(device=self.dev).manual_seed(a.seed + 11)
        start = int(torch.randint(0, a.n - a.m, (1,), generator=g, device=self.dev))
        d_q = self.d_text[start:start + a.m].clone()
        at = torch.arange(25, a.m, 50, device=self.dev)
        at = at + torch.randint(-10, 11, at.shape, generator=g, device=self.dev)
        d_q[at] = self.other_symbol(d_q[at])
        out = []
        for L in (16, 20, 32):
            for max_occ in (0, 64):
                fn, info, keepalive = self.mems_fn(d_q, L, max_occ, "auto")
                seeds, locate, hits = self.parts(d_q, L, max_occ)
                assert hits == info[1], "the parts' hits are not the candidates"
                waits = {}
                for name, f in (("mems", fn), ("seeds", seeds), ("locate", locate)):
                    before = self.b.L.sa_host_syncs()
                    f()
                    waits[name] = int(self.b.L.sa_host_syncs() - before)
                r = self.record(timed(torch, {"mems": fn, "seeds": seeds, "locate": locate}, a.runs, a.warmup), info)
                t = r["mems"]["ms_median"]
                out.append({"L": L, "max_occ": max_occ, "m": a.m, "mems": info[0], "candidates": info[1],
                            "skipped": info[2], "host_waits": waits, "calls": r, "seed_share": r["seeds"]["ms_median"] / t,
                            "locate_share": r["locate"]["ms_median"] / t,
                            "after_seeds_over_locate": (t - r["seeds"]["ms_median"]) / r["locate"]["ms_median"]})
                del keepalive
                torch.cuda.empty_cache()
        return out

    def slices(self):
        torch, a = self.torch, self.a
        out = []
        for m in (1 << 16, 1 << 20):
            start = a.n // 3
            d_q = self.d_text[start:start + m].clone()
            fns, info = {}, None
            keep = []
            for mode in ("auto", "lane", "wave"):
                fns[mode], i2, k = self.mems_fn(d_q, 20, 0, mode)
                keep.append(k)
                assert info is None or i2 == info
                info = i2
            ref = None
            for mode, k in zip(fns, keep):   # the three modes agree before anything is timed
                fns[mode]()
                torch.cuda.synchronize()
                cur = (k[0].clone(), k[1][:info[0]].clone(), k[2][:info[0]].clone())
                assert ref is None or all(torch.equal(x, y) for x, y in zip(ref, cur)), f"{mode} differs from auto"
                ref = cur
            longest = int(ref[2].max())
            r = self.record(timed(torch, fns, a.runs, a.warmup), info)
            out.append({"m": m, "L": 20, "mems": info[0], "candidates": info[1], "longest": longest, "calls": r})
            torch.cuda.empty_cache()
        return out

    def blocks(self):
        torch, a = self.torch, self.a
        out = []
        for B in a.blocks:
            k = a.m // (B + 1)
            g = torch.Generator(device=self.dev).manual_seed(a.seed + B)
            start = torch.randint(0, a.n - B - 1, (k,), generator=g, device=self.dev)
            idx = (start[:, None] + torch.arange(B + 1, device=self.dev)[None, :])
            d_q = self.d_text[idx.reshape(-1)].contiguous()
            sep = torch.arange(k, device=self.dev) * (B + 1) + B          # the byte after each block: changed
            d_q[sep] = self.other_symbol(d_q[sep])
            fns, info = {}, None
            keep = []
            for mode in ("lane", "wave", "auto"):
                fns[mode], info, kk = self.mems_fn(d_q, 20, 64, mode)
                keep.append(kk)
            r = self.record(timed(torch, fns, a.runs, a.warmup), info)
            out.append({"block_bytes": B, "blocks": k, "L": 20, "max_occ": 64, "mems": info[0], "candidates": info[1],
                        "calls": r, "wave_minus_lane_ms": r["wave"]["ms_median"] - r["lane"]["ms_median"]})
            del keep
            torch.cuda.empty_cache()
        return out


def main():
    a = parse()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mem.py needs an MI355X: no HIP device is visible")
    from hpc_suffix_array_amd import DeviceBuilder, _native as N
    dev = torch.device("cuda", 0)
    b = DeviceBuilder(a.n)
    d_text = torch.empty(a.n, dtype=torch.uint8, device=dev)
    b.generate_text(d_text, a.n, b"ACGT", seed=a.seed)
    d_sa = torch.empty(a.n, dtype=torch.int32, device=dev)
    st = b.build(d_text, a.n, d_sa)
    torch.cuda.synchronize()
    out = {"bench": "mem", "n": a.n, "kind": "dna", "seed": a.seed, "src_hash": N.source_hash(),
           "cus": torch.cuda.get_device_properties(0).multi_processor_count, "build_ms": st["total_ms"]}
    bench = Bench(torch, a, b, d_text, d_sa)
    if "subst" in a.workloads:
        out["subst"] = bench.subst()
    if "slice" in a.workloads:
        out["slice"] = bench.slices()
    if "blocks" in a.workloads:
        out["blocks"] = bench.blocks()
    b.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
