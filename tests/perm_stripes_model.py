"""The level-1 plan of the coalesced permutations (the checker's two passes,
LCP's PHI / ISA + 1 / PLCP and the inverse SA), restated in numpy: plan_check,
pad_elems and plan_stripes of hpc_suffix_array_amd/csrc/sa_build.hip, and the
fill of every (bin, stripe) region that k_chk_bin (sa_check.h) writes.

The GPU tests use it to prove, before they call the library, that an input
takes the path it is meant to take (striped, unstriped, a stripe at exactly
its capacity, a stripe that overflows).  It only chooses inputs: no result of
the library is ever compared with it.
"""
from collections import namedtuple

import numpy as np

SUB_A = 14          # kChkSubA = kPermSub: sub-bin bits of pass A, PHI, ISA + 1, PLCP, the inverse
SUB_B = 13          # kChkSubB: sub-bin bits of the checker's pass B (n <= 2^31)
STRIPES = 8         # kChkStripes
TILE = 1024 * 8     # kChkBlock * kChkItems: level-1 elements per workgroup (256 bins)
TILE_WIDE = 1024 * 7   # k_chk_bin with 512 / 1024 bins (tune bits 20-23 = 2 / 1)
STRIPE_MIN_N = 1 << 24

Plan = namedtuple("Plan", "s1 s2 nb1 nsub")
Stripes = namedtuple("Stripes", "st scap")


def align_up(x: int, a: int) -> int:
    return (x + a - 1) // a * a


def pad_elems(cap: int) -> int:
    """keys[0] capacity (elements) of a context created for ``cap`` symbols."""
    m = align_up(max(cap, 1), 64)
    if (1 << 26) <= cap <= (1 << 31):
        return align_up(cap + cap // 8 + (1 << 22), 64)
    return m


def plan_check(n: int, s2: int = SUB_A, b1: int = 8) -> Plan:
    lg = (n - 1 if n > 1 else 1).bit_length()
    s1 = max(s2, lg - b1 if lg > b1 else 0)
    nb1 = (n + (1 << s1) - 1) >> s1
    return Plan(s1, s2, nb1, 1 << (s1 - s2))


def plan_stripes(cap: int, n: int, p: Plan, want: int = STRIPES) -> Stripes:
    """``cap``: what the context was created (or last grown) for, not n."""
    if want <= 1 or n < STRIPE_MIN_N:
        return Stripes(1, 0)
    per = ((1 << p.s1) + want - 1) // want
    scap = per + max(2048, (1 << p.s1) // 128)
    if p.nb1 * want * scap > pad_elems(cap):
        return Stripes(1, 0)
    return Stripes(want, scap)


def level1_tile(p: Plan) -> int:
    """Elements per level-1 workgroup: k_chk_bin's NB follows the bin count."""
    return TILE if p.nb1 <= 256 else TILE_WIDE


def region_fill(dest: np.ndarray, p: Plan, st: int = STRIPES, tile: int = None) -> np.ndarray:
    """[nb1, st] pairs that level 1 sends to each (bin, stripe) region:
    element e (in source order) has stripe (e // tile) mod st and bin
    dest[e] >> s1.  Every dest must be < n."""
    tile = level1_tile(p) if tile is None else tile
    d = np.asarray(dest).astype(np.int64)
    q = (np.arange(d.size, dtype=np.int64) // tile) % st
    return np.bincount((d >> p.s1) * st + q, minlength=p.nb1 * st).reshape(p.nb1, st)


def is_striped(cap: int, n: int, s2: int = SUB_A, b1: int = 8) -> bool:
    return plan_stripes(cap, n, plan_check(n, s2, b1)).st > 1


# --- the inputs of the tests ------------------------------------------------
PERIOD = 256


def periodic_text(reps: int) -> np.ndarray:
    """bytes(range(256)) * reps."""
    return np.tile(np.arange(PERIOD, dtype=np.uint8), reps)


def periodic_sa(reps: int) -> np.ndarray:
    """SA[c reps + k] = c + 256 (reps - 1 - k): the suffixes that start with
    symbol c, the shortest first (each is a prefix of the next longer one)."""
    r = np.arange(PERIOD * reps, dtype=np.int64)
    c, k = r // reps, r % reps
    return (c + PERIOD * (reps - 1 - k)).astype(np.uint32)


def periodic_lcp(reps: int) -> np.ndarray:
    """LCP[c reps + k] = 0 for k = 0, else 256 k - c: the whole shorter suffix."""
    r = np.arange(PERIOD * reps, dtype=np.int64)
    c, k = r // reps, r % reps
    return np.where(k == 0, 0, PERIOD * k - c).astype(np.uint32)


def swapped_identity(n: int, k: int, a: int = 1 << 16, b: int = 1 << 13) -> np.ndarray:
    """The identity on n with p[a : a + k] and p[b : b + k] exchanged."""
    p = np.arange(n, dtype=np.uint32)
    p[a:a + k] = np.arange(b, b + k, dtype=np.uint32)
    p[b:b + k] = np.arange(a, a + k, dtype=np.uint32)
    return p
