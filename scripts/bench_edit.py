#!/usr/bin/env python3
"""Time of the k-difference search (sa_edit_device) on one MI355X, next to its
parts measured in the same process (sa_find_device on the pieces,
sa_locate_device on their intervals) and next to sa_hamming_device on the same
reads and k: hamming has the same seeds and strictly less verification, so it
is a floor and the ratio is the price of indels.  There is no pass/fail
number: the tables say what was measured.

The text is random DNA (2^28 by default), generated on the device, its SA built
in place.  Workloads:

    reads    --nq reads of 32, 100 and 250 bytes read from the text with k
             planted edits (substitutions, insertions and deletions in turn).
             For each length k goes up through --ks until the candidates pass
             --stop-candidates (2^27); that last k is still measured when its
             candidates are at most --max-candidates.  Checked first: every
             planted end is listed with a distance of at most k.
    long     a few thousand reads of 1024 and 8192 bytes, k = 3: a lane runs
             the whole band of a long pattern by itself, and this is where a
             wavefront path would have to pay.

Each call is warmed up and timed alone between two device events, --runs
times, the calls of one workload alternating run by run.  Reported per call:
median, minimum and maximum in ms; ns per candidate and per end; the host
waits of one call.  Prints one JSON line and writes it to --out when given.
With no GPU the script fails.

    python scripts/bench_edit.py [--n 268435456] [--nq 1048576] [--runs 5] [--out profiles/bench_edit.json]
    python scripts/bench_edit.py --n 67108864 --nq 262144 --workloads reads --lengths 100 --ks 3 --runs 2 --warmup 1   # a short run for a kernel trace
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
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workloads", nargs="+", default=["reads", "long"], choices=["reads", "long"])
    ap.add_argument("--lengths", nargs="+", type=int, default=[32, 100, 250])
    ap.add_argument("--ks", nargs="+", type=int, default=[1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 18, 20, 24, 31])
    ap.add_argument("--long-lengths", nargs="+", type=int, default=[1024, 8192])
    ap.add_argument("--long-nq", type=int, default=4096)
    ap.add_argument("--stop-candidates", type=int, default=1 << 27)
    ap.add_argument("--max-candidates", type=int, default=1 << 29)
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
        """nq reads of m bytes read from the text, each with k edits at
        distinct bytes, read q's j-th edit of kind (q + j) mod 3: a
        substituted byte, a byte the text does not have, a text byte the read
        skips.  (d_pat, d_off, the end of the text each was read from)."""
        torch, n = self.torch, self.a.n
        g = torch.Generator(device=self.dev).manual_seed(seed)
        start = torch.randint(0, n - m - k - 1, (nq,), generator=g, device=self.dev)
        ar = torch.arange(m, device=self.dev)
        d_pat = torch.empty(nq * m, dtype=torch.uint8, device=self.dev)
        rows = d_pat.view(nq, m)
        end = torch.empty(nq, dtype=torch.int64, device=self.dev)
        step = max(1, (1 << 24) // m)
        for c0 in range(0, nq, step):
            c1 = min(nq, c0 + step)
            cnt = c1 - c0
            where = torch.rand(cnt, m, generator=g, device=self.dev).topk(k, dim=1, largest=False).indices
            kind = (torch.arange(c0, c1, device=self.dev)[:, None] + torch.arange(k, device=self.dev)[None, :]) % 3
            # the text byte behind read byte i is start + i + (deletions at or in front of i) - (insertions in front of i)
            mark = torch.zeros(cnt, m + 1, dtype=torch.int32, device=self.dev)
            mark.scatter_add_(1, where, (kind == 2).int())
            mark.scatter_add_(1, where + 1, -(kind == 1).int())
            full = mark.cumsum(1)
            shift = full[:, :m]
            chunk = self.d_text[start[c0:c1, None] + ar[None, :] + shift]
            changed = kind != 2
            qq = torch.arange(cnt, device=self.dev)[:, None].expand(cnt, k)[changed]
            xx = where[changed]
            chunk[qq, xx] = self.other_symbol(chunk[qq, xx])
            rows[c0:c1] = chunk
            end[c0:c1] = start[c0:c1] + m + full[:, m]      # m + deletions - insertions text bytes
        d_off = torch.arange(nq + 1, dtype=torch.int64, device=self.dev) * m
        return d_pat, d_off, end

    def edit_fn(self, d_pat, d_off, nq, k):
        torch = self.torch
        d_out = torch.empty(nq + 1, dtype=torch.int64, device=self.dev)
        args = (self.d_text, self.a.n, self.d_sa, d_pat, d_pat.numel(), d_off, nq, k, d_out)
        info = self.b.edit(*args, None, None, None, 0, stream=self.sptr)
        d_end = torch.empty(max(info[0], 1), dtype=torch.int32, device=self.dev)
        d_start = torch.empty(max(info[0], 1), dtype=torch.int32, device=self.dev)
        d_dist = torch.empty(max(info[0], 1), dtype=torch.uint8, device=self.dev)

        def fn():
            self.b.edit(*args, d_end, d_start, d_dist, info[0], stream=self.sptr)

        def ends_only():
            self.b.edit(*args, d_end, None, None, info[0], stream=self.sptr)
        return fn, ends_only, info, (d_out, d_end, d_start, d_dist)

    def hamming_fn(self, d_pat, d_off, nq, k):
        torch = self.torch
        d_out = torch.empty(nq + 1, dtype=torch.int64, device=self.dev)
        args = (self.d_text, self.a.n, self.d_sa, d_pat, d_pat.numel(), d_off, nq, k, d_out)
        info = self.b.hamming(*args, None, None, 0, stream=self.sptr)
        d_pos = torch.empty(max(info[0], 1), dtype=torch.int32, device=self.dev)
        d_dist = torch.empty(max(info[0], 1), dtype=torch.uint8, device=self.dev)

        def fn():
            self.b.hamming(*args, d_pos, d_dist, info[0], stream=self.sptr)
        return fn, info, (d_out, d_pos, d_dist)

    def parts(self, d_pat, d_off, nq, m, k, cap):
        """find on the pieces alone and locate (SA order) of their intervals
        alone, when the candidates are at most cap."""
        torch, n = self.torch, self.a.n
        np_ = nq * (k + 1)
        bj = torch.tensor([j * m // (k + 1) for j in range(k + 1)], dtype=torch.int64, device=self.dev)
        d_poff = torch.cat([(d_off[:nq, None] + bj[None, :]).reshape(-1), d_off[nq:nq + 1]]).contiguous()
        d_lo = torch.empty(np_, dtype=torch.int32, device=self.dev)
        d_hi = torch.empty(np_, dtype=torch.int32, device=self.dev)

        def find():
            self.b.find(self.d_text, n, self.d_sa, d_pat, d_pat.numel(), d_poff, np_, d_lo, d_hi, stream=self.sptr)
        find()
        torch.cuda.synchronize()
        total = int((u32(d_hi) - u32(d_lo)).sum())
        if total > cap:
            return find, None, total
        d_coff = torch.empty(np_ + 1, dtype=torch.int64, device=self.dev)
        d_cand = torch.empty(max(total, 1), dtype=torch.int32, device=self.dev)

        def locate():
            self.b.locate(n, self.d_sa, d_lo, d_hi, np_, d_coff, d_cand, total, order="sa", stream=self.sptr)
        locate()
        torch.cuda.synchronize()
        return find, locate, total

    def measure(self, nq, m, k, seed):
        torch, a = self.torch, self.a
        d_pat, d_off, end = self.patterns(nq, m, k, seed)
        find, locate, cands = self.parts(d_pat, d_off, nq, m, k, a.max_candidates)
        row = {"m": m, "k": k, "nq": nq, "pieces": nq * (k + 1), "candidates": cands}
        if locate is None:
            row["measured"] = "not measured: the candidates exceed --max-candidates"
            row["calls"] = timed(torch, {"find_pieces": find}, a.runs, a.warmup)
            return row
        fn, ends_only, info, outs = self.edit_fn(d_pat, d_off, nq, k)
        assert info[1] == cands and info[2] == nq * (k + 1)
        before = self.b.L.sa_host_syncs()
        fn()
        row["host_waits"] = int(self.b.L.sa_host_syncs() - before)
        torch.cuda.synchronize()
        # every planted end is listed, with a distance of at most k
        d_out, d_end, d_start, d_dist = outs
        q = torch.repeat_interleave(torch.arange(nq, device=self.dev), d_out[1:] - d_out[:-1])
        mine = q * (a.n + 1) + u32(d_end[:info[0]])
        planted = torch.arange(nq, device=self.dev) * (a.n + 1) + end
        at = torch.searchsorted(mine, planted).clamp(max=max(info[0] - 1, 0))
        assert bool((mine[at] == planted).all()), "a planted end is missing"
        assert int(d_dist[:info[0]].max()) <= k and bool((u32(d_start[:info[0]]) <= u32(d_end[:info[0]])).all())
        row["checked"] = "every planted end listed, distances within k"
        hfn, hinfo, houts = self.hamming_fn(d_pat, d_off, nq, k)
        assert hinfo[1] == cands
        r = timed(torch, {"edit": fn, "edit_ends_only": ends_only, "hamming": hfn, "find_pieces": find,
                          "locate_pieces": locate}, a.runs, a.warmup)
        for v in r.values():
            v["ns_per_candidate"] = v["ms_median"] * 1e6 / max(cands, 1)
            v["ns_per_end"] = v["ms_median"] * 1e6 / max(info[0], 1)
        parts = r["find_pieces"]["ms_median"] + r["locate_pieces"]["ms_median"]
        row.update({"ends": info[0], "hamming_hits": hinfo[0], "calls": r,
                    "after_parts_ms": r["edit"]["ms_median"] - parts,
                    "hamming_after_parts_ms": r["hamming"]["ms_median"] - parts,
                    "edit_over_hamming": r["edit"]["ms_median"] / max(r["hamming"]["ms_median"], 1e-9)})
        del outs, houts
        torch.cuda.empty_cache()
        return row

    def reads(self, flush):
        a = self.a
        out = []
        for m in a.lengths:
            for k in a.ks:
                if m <= k:
                    break
                row = self.measure(a.nq, m, k, a.seed + 1000 * m + k)
                out.append(row)
                flush(out)
                if row["candidates"] > a.stop_candidates:
                    break
        return out

    def long(self):
        a = self.a
        return [self.measure(a.long_nq, m, 3, a.seed + 7 * m) for m in a.long_lengths]


def main():
    a = parse()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_edit.py needs an MI355X: no HIP device is visible")
    from hpc_suffix_array_amd import DeviceBuilder, _native as N
    dev = torch.device("cuda", 0)
    b = DeviceBuilder(a.n)
    d_text = torch.empty(a.n, dtype=torch.uint8, device=dev)
    b.generate_text(d_text, a.n, b"ACGT", seed=a.seed)
    d_sa = torch.empty(a.n, dtype=torch.int32, device=dev)
    st = b.build(d_text, a.n, d_sa)
    torch.cuda.synchronize()
    out = {"bench": "edit", "n": a.n, "kind": "dna", "seed": a.seed, "src_hash": N.source_hash(),
           "cus": torch.cuda.get_device_properties(0).multi_processor_count, "build_ms": st["total_ms"]}
    bench = Bench(torch, a, b, d_text, d_sa)

    def flush(reads=None):
        if reads is not None:
            out["reads"] = reads
        line = json.dumps(out)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return line
    if "long" in a.workloads:
        out["long"] = bench.long()
        flush()
    if "reads" in a.workloads:
        out["reads"] = bench.reads(flush)
    b.close()
    print(flush())


if __name__ == "__main__":
    main()
