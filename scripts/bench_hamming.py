#!/usr/bin/env python3
"""Time of the k-mismatch search (sa_hamming_device) on one MI355X, next to its
parts measured in the same process: sa_find_device on the pieces,
sa_locate_device on their intervals, and a torch composition of what comes
after them (window gather, compare, sum, mask, unique, sort) on the same
candidate list.  There is no pass/fail number: the tables say what was
measured.

The text is random DNA (2^28 by default), generated on the device, its SA built
in place.  Workloads:

    reads    --nq patterns of 32, 64 and 128 bytes cut from the text with
             exactly k substitutions, k = 0 .. 4.  The outputs are checked
             first: k = 0 against find + locate on the same patterns, every k
             against the torch verification of the same candidates.  A
             combination whose pieces have more than --max-candidates exact
             occurrences (short pieces in a long text: 8 bytes of DNA occur
             4096 times in 2^28) is counted by find alone and recorded as not
             measured.
    lane     patterns of 64 .. 16,384 bytes (2^24 pattern bytes a batch), k = 3,
             under lane / wave / auto: where lane and wave cross is where a
             lane should hand over (kHamLaneBytes of csrc/sa_hamming.h).

Each call is warmed up and timed alone between two device events, --runs
times, the calls of one workload alternating run by run.  Reported per call:
median, minimum and maximum in ms; ns per candidate and per hit.  Prints one
JSON line and writes it to --out when given.  With no GPU the script fails.

    python scripts/bench_hamming.py [--n 268435456] [--nq 1048576] [--runs 10] [--out profiles/bench_hamming.json]
    python scripts/bench_hamming.py --workloads reads --lengths 64 --ks 2 --runs 3 --warmup 1   # a short run for a kernel trace
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
    ap.add_argument("--nq", type=int, default=1 << 20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workloads", nargs="+", default=["reads", "lane"], choices=["reads", "lane"])
    ap.add_argument("--lengths", nargs="+", type=int, default=[32, 64, 128])
    ap.add_argument("--ks", nargs="+", type=int, default=[0, 1, 2, 3, 4])
    ap.add_argument("--lane-lengths", nargs="+", type=int, default=[64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384])
    ap.add_argument("--lane-bytes", type=int, default=1 << 24)
    ap.add_argument("--max-candidates", type=int, default=1 << 29)
    ap.add_argument("--torch-candidates", type=int, default=1 << 27,
                    help="the torch composition is timed up to this many candidates")
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


def u32(x):
    """The uint32 bits of an int32 tensor as int64."""
    return x.long() & 0xFFFFFFFF


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

    def patterns(self, nq, m, k, seed):
        """nq patterns of m bytes cut from the text, each with exactly k
        substitutions at distinct bytes; (d_pat, d_off, starts)."""
        torch, n = self.torch, self.a.n
        g = torch.Generator(device=self.dev).manual_seed(seed)
        start = torch.randint(0, n - m, (nq,), generator=g, device=self.dev)
        ar = torch.arange(m, device=self.dev)
        d_pat = torch.empty(nq * m, dtype=torch.uint8, device=self.dev)
        rows = d_pat.view(nq, m)
        step = max(1, (1 << 26) // m)
        for c0 in range(0, nq, step):
            rows[c0:c0 + step] = self.d_text[start[c0:c0 + step, None] + ar[None, :]]
        if k:
            # k distinct bytes per pattern: the k smallest of m random keys
            where = torch.rand(nq, m, generator=g, device=self.dev).topk(k, dim=1, largest=False).indices
            flat = (torch.arange(nq, device=self.dev)[:, None] * m + where).reshape(-1)
            d_pat[flat] = self.other_symbol(d_pat[flat])
        d_off = torch.arange(nq + 1, dtype=torch.int64, device=self.dev) * m
        return d_pat, d_off, start

    def sized(self, d_pat, d_off, nq, k, mode, cap=0):
        torch = self.torch
        d_out = torch.empty(nq + 1, dtype=torch.int64, device=self.dev)
        info = self.b.hamming(self.d_text, self.a.n, self.d_sa, d_pat, d_pat.numel(), d_off, nq, k, d_out, None, None, 0,
                              max_candidates=cap, mode=mode, stream=self.sptr)
        d_pos = torch.empty(max(info[0], 1), dtype=torch.int32, device=self.dev)
        d_dist = torch.empty(max(info[0], 1), dtype=torch.uint8, device=self.dev)
        return d_out, d_pos, d_dist, info

    def hamming_fn(self, d_pat, d_off, nq, k, mode):
        d_out, d_pos, d_dist, info = self.sized(d_pat, d_off, nq, k, mode)

        def fn():
            self.b.hamming(self.d_text, self.a.n, self.d_sa, d_pat, d_pat.numel(), d_off, nq, k, d_out, d_pos, d_dist,
                           info[0], mode=mode, stream=self.sptr)
        return fn, info, (d_out, d_pos, d_dist)

    def pieces(self, d_off, nq, m, k):
        """The piece offsets of nq patterns of m bytes each."""
        torch = self.torch
        b = torch.tensor([j * m // (k + 1) for j in range(k + 1)], dtype=torch.int64, device=self.dev)
        poff = (d_off[:nq, None] + b[None, :]).reshape(-1)
        return torch.cat([poff, d_off[nq:nq + 1]]).contiguous(), b

    def parts(self, d_pat, d_off, nq, m, k, cap):
        """find on the pieces alone and locate (SA order) of their intervals
        alone; the candidates with their owners when they are at most cap."""
        torch, n = self.torch, self.a.n
        np_ = nq * (k + 1)
        d_poff, bj = self.pieces(d_off, nq, m, k)
        d_lo = torch.empty(np_, dtype=torch.int32, device=self.dev)
        d_hi = torch.empty(np_, dtype=torch.int32, device=self.dev)

        def find():
            self.b.find(self.d_text, n, self.d_sa, d_pat, d_pat.numel(), d_poff, np_, d_lo, d_hi, stream=self.sptr)
        find()
        torch.cuda.synchronize()
        cnt = u32(d_hi) - u32(d_lo)
        total = int(cnt.sum())
        if total > cap:
            return find, None, total, None
        d_coff = torch.empty(np_ + 1, dtype=torch.int64, device=self.dev)
        d_cand = torch.empty(max(total, 1), dtype=torch.int32, device=self.dev)

        def locate():
            self.b.locate(n, self.d_sa, d_lo, d_hi, np_, d_coff, d_cand, total, order="sa", stream=self.sptr)
        locate()
        torch.cuda.synchronize()
        return find, locate, total, (cnt, d_cand, bj)

    def torch_verify(self, d_pat, nq, m, k, cand):
        """Steps 5 to 9 in torch on the same candidates: the sorted unique keys
        ((q n + p) 256 + d) of the candidates that are valid and within k."""
        torch, n = self.torch, self.a.n
        cnt, d_cand, bj = cand
        assert nq * n * 256 < (1 << 62)
        owner = torch.repeat_interleave(torch.arange(cnt.numel(), device=self.dev), cnt)
        rows = d_pat.view(nq, m)
        ar = torch.arange(m, device=self.dev)
        keys = []
        step = max(1, (1 << 28) // m)
        for c0 in range(0, owner.numel(), step):
            g = owner[c0:c0 + step]
            q, j = g // (k + 1), g % (k + 1)
            p = u32(d_cand[c0:c0 + step]) - bj[j]
            valid = (p >= 0) & (p + m <= n)
            pc = p.clamp(0, n - m)
            d = (self.d_text[pc[:, None] + ar[None, :]] != rows[q]).sum(dim=1)
            keep = valid & (d <= k)
            keys.append(((q * n + p) * 256 + d)[keep])
        return torch.unique(torch.cat(keys), sorted=True)

    def our_keys(self, outs, nq, total):
        torch, n = self.torch, self.a.n
        d_out, d_pos, d_dist = outs
        q = torch.repeat_interleave(torch.arange(nq, device=self.dev), d_out[1:] - d_out[:-1])
        return (q * n + u32(d_pos[:total])) * 256 + d_dist[:total].to(torch.int64)

    def reads(self):
        torch, a = self.torch, self.a
        out = []
        for m in a.lengths:
            for k in a.ks:
                nq = a.nq
                d_pat, d_off, start = self.patterns(nq, m, k, a.seed + 1000 * m + k)
                find, locate, cands, cand = self.parts(d_pat, d_off, nq, m, k, a.max_candidates)
                row = {"m": m, "k": k, "nq": nq, "pieces": nq * (k + 1), "candidates": cands}
                if locate is None:
                    row["measured"] = "not measured: the candidates exceed --max-candidates"
                    row["calls"] = timed(torch, {"find_pieces": find}, a.runs, a.warmup)
                    out.append(row)
                    continue
                fn, info, outs = self.hamming_fn(d_pat, d_off, nq, k, "auto")
                assert info[1] == cands and info[2] == nq * (k + 1)
                before = self.b.L.sa_host_syncs()
                fn()
                row["host_waits"] = int(self.b.L.sa_host_syncs() - before)
                torch.cuda.synchronize()
                # every planted occurrence is listed with distance k
                mine = self.our_keys(outs, nq, info[0])
                planted = (torch.arange(nq, device=self.dev) * a.n + start) * 256 + k
                at = torch.searchsorted(mine, planted).clamp(max=max(info[0] - 1, 0))
                assert bool((mine[at] == planted).all()), "a planted occurrence is missing"
                ref = self.torch_verify(d_pat, nq, m, k, cand)
                assert torch.equal(mine, ref), f"m {m} k {k}: the output differs from the torch verification"
                if k == 0:
                    d_lo = torch.empty(nq, dtype=torch.int32, device=self.dev)
                    d_hi = torch.empty(nq, dtype=torch.int32, device=self.dev)
                    self.b.find(self.d_text, a.n, self.d_sa, d_pat, d_pat.numel(), d_off, nq, d_lo, d_hi, stream=self.sptr)
                    d_o = torch.empty(nq + 1, dtype=torch.int64, device=self.dev)
                    d_p = torch.empty(max(info[0], 1), dtype=torch.int32, device=self.dev)
                    tot = self.b.locate(a.n, self.d_sa, d_lo, d_hi, nq, d_o, d_p, info[0], stream=self.sptr)
                    assert tot == info[0] and torch.equal(d_o, outs[0]) and torch.equal(d_p[:tot], outs[1][:tot])
                    assert int(outs[2][:tot].max()) == 0
                row["checked"] = "torch verification" + (", find + locate" if k == 0 else "")
                fns = {"hamming": fn, "find_pieces": find, "locate_pieces": locate}
                r = timed(torch, fns, a.runs, a.warmup)
                if cands <= a.torch_candidates:
                    r.update(timed(torch, {"torch_steps_5_to_9": lambda: self.torch_verify(d_pat, nq, m, k, cand)},
                                   min(a.runs, 3), 1))
                else:
                    row["torch_steps_5_to_9"] = "not measured: more candidates than --torch-candidates"
                for v in r.values():
                    v["ns_per_candidate"] = v["ms_median"] * 1e6 / max(cands, 1)
                    v["ns_per_hit"] = v["ms_median"] * 1e6 / max(info[0], 1)
                t = r["hamming"]["ms_median"]
                row.update({"hits": info[0], "calls": r,
                            "after_parts_ms": t - r["find_pieces"]["ms_median"] - r["locate_pieces"]["ms_median"]})
                out.append(row)
                del outs, cand, ref, mine
                torch.cuda.empty_cache()
        return out

    def lane(self):
        torch, a = self.torch, self.a
        out = []
        k = 3
        for m in a.lane_lengths:
            nq = max(64, a.lane_bytes // m)
            d_pat, d_off, start = self.patterns(nq, m, k, a.seed + 7 * m)
            fns, info, keep, ref = {}, None, [], None
            for mode in ("lane", "wave", "auto"):
                fns[mode], i2, o = self.hamming_fn(d_pat, d_off, nq, k, mode)
                keep.append(o)
                assert info is None or i2 == info
                info = i2
                fns[mode]()
                torch.cuda.synchronize()
                cur = self.our_keys(o, nq, info[0])
                assert ref is None or torch.equal(ref, cur), f"{mode} differs from lane"
                ref = cur
            r = timed(torch, fns, a.runs, a.warmup)
            for v in r.values():
                v["ns_per_candidate"] = v["ms_median"] * 1e6 / max(info[1], 1)
                v["ns_per_hit"] = v["ms_median"] * 1e6 / max(info[0], 1)
            out.append({"m": m, "k": k, "nq": nq, "hits": info[0], "candidates": info[1], "calls": r,
                        "wave_minus_lane_ms": r["wave"]["ms_median"] - r["lane"]["ms_median"]})
            del keep
            torch.cuda.empty_cache()
        return out


def main():
    a = parse()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_hamming.py needs an MI355X: no HIP device is visible")
    from hpc_suffix_array_amd import DeviceBuilder, _native as N
    dev = torch.device("cuda", 0)
    b = DeviceBuilder(a.n)
    d_text = torch.empty(a.n, dtype=torch.uint8, device=dev)
    b.generate_text(d_text, a.n, b"ACGT", seed=a.seed)
    d_sa = torch.empty(a.n, dtype=torch.int32, device=dev)
    st = b.build(d_text, a.n, d_sa)
    torch.cuda.synchronize()
    out = {"bench": "hamming", "n": a.n, "kind": "dna", "seed": a.seed, "src_hash": N.source_hash(),
           "cus": torch.cuda.get_device_properties(0).multi_processor_count, "build_ms": st["total_ms"],
           "lane_bytes": N.HAMMING_LANE_BYTES}
    bench = Bench(torch, a, b, d_text, d_sa)

    def flush():
        line = json.dumps(out)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return line
    if "lane" in a.workloads:
        out["lane"] = bench.lane()
        flush()
    if "reads" in a.workloads:
        out["reads"] = bench.reads()
    b.close()
    print(flush())


if __name__ == "__main__":
    main()
