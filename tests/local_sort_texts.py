"""Texts whose windows the fixed-span local sort (sa_bucket.h k_bucket_sort)
finds hard, and a numpy model of the bucketed first round's window layout.

Uniform text of a size a CPU oracle sorts has no one-bucket window: a window
holds one bucket only when wb[j + 1] - wb[j] == 1 (k_window_starts_tab), empty
buckets count in that difference, so a run of consecutive buckets must hold
about a window stride (1024 suffixes) each.  anchored_text() builds such runs
from blocks:

  anchor    `alen` copies of one symbol a; the pattern a^alen occurs nowhere
            else in the text (every other position that is a multiple of alen
            inside its block, and every block's last position, avoids a), so
            the suffixes whose first s symbols start with the anchor are the
            anchored blocks' starts and nothing else: bucket sizes are exact
  selector  the rest of D (the bucket); never starts with a, which would
            extend the anchor run
  neck      the key bits that pick the sub-bucket, drawn round-robin from a
            per-bucket set of T values: every one of the T sub-buckets holds
            floor or ceil of count / T keys
  tail      the key bits below the sub-bucket (random, or one of `lows`
            values: large tie groups), then random filler to the block's end

The blocks are shuffled; the rest of the text is filler blocks, random or --
`dense` -- 4-block pieces each written twice, which leaves more than
n / kSparseDiv suffixes in tie groups after round 1 (the dense second launch
of the local sort) without long repeats (the oracle's rounds stay few).

WindowModel restates plan_bucketed (sa_round1.h), the key layout of
tests/test_key1_layout.py (key1, bucket = (D cmul) >> bsh, bucket_dmin) and
k_window_starts_tab / k_window_list / k_window_split in numpy: bucket sizes,
ws / wb, the one-bucket windows, their sizes, each one's largest sub-bucket
(the top kSubBits bits of the bits1-bit bucket-relative key) and the tie
groups.  Everything here runs without a GPU.

The last section models the second bucket pass (sa_split.h k_split_seg) for
tests/test_gpu_second_pass.py: host_plan / plan_bucketed take the bucket bits
that debug bb17 / bb18 force, second_pass_units() restates the pass's unit
numbering, the units' queues and k_xq_dh's sub-regions, and sp_text() builds
the texts whose segments reach the pass's edges
(tests/test_second_pass_texts.py asserts that on the CPU).
"""
import functools

import numpy as np

# sa_bucket.h
K_WIN_STRIDE = 1024
K_BS_CAP = 9216
K_SUB_BITS = 11
K_MAX_SUB = 64
K_LOW_MAX = 18          # 32 - kSlotBits
K_WAVE_ROW = 64 * 18    # one wave's slots of a window (kWave * kBsItems): the wfull edge
K_SPARSE_DIV = 8        # sa_build.hip
K_MAX_K = 64            # sa_kernels.h

ALPHABETS = {
    "dna": b"ACGT",
    "alnum": bytes(sorted(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789")),
    "byte256": bytes(range(256)),
}
# largest-sub-bucket classes of a one-bucket window: 4-, 8-, 12-, 16-input
# networks, the LDS insertion sort, the clustered-window retry (> kMaxSub)
SUB_CLASSES = ((1, 4), (5, 8), (9, 12), (13, 16), (17, K_MAX_SUB), (K_MAX_SUB + 1, K_BS_CAP))


# --------------------------------------------------------------------------
# the host's plan (sa_build.hip min_chars, sa_round1.h plan_bucketed)
# --------------------------------------------------------------------------
def _max_chars(base):
    k, prod = 0, 1
    while prod <= (2 ** 64 - 1) // base:
        prod *= base
        k += 1
    return k


def min_chars(sigma, n):
    kmax = _max_chars(sigma + 1)
    k, p = 1, sigma
    while p < n * 512 and k < kmax:
        p *= sigma
        k += 1
    return k


def plan_bucketed(sigma, n, K, cmp=1, bb=None):
    """BucketPlan of one GPU (world 1) as a dict, or None.  bb: the bucket
    bits debug bb17 / bb18 force (never fewer than the size gives)."""
    if sigma < 2 or n < 2:
        return None
    ib = (n - 1).bit_length()
    bb = max(min(max(16, ib - 13 if ib > 13 else 0), 18), min(bb or 0, 18))
    ps, s = 1, 0
    while ps < (1 << bb):
        ps *= sigma
        s += 1
    while ps % (1 << bb) != 0 and ps < (64 << bb) and s + 1 < K and ps * sigma <= (1 << 32):
        ps *= sigma
        s += 1
    if ps > (1 << 32) or K <= s or K > K_MAX_K:
        return None
    bd = (ps - 1).bit_length()
    per = (ps + (1 << bb) - 1) >> bb
    span = per.bit_length() + 1
    for R in range(K - s, 0, -1):
        pr = sigma ** R
        lowmax = pr - 1 if cmp == 2 else 2 * pr - 1 if cmp else s + (pr - 1) * (R + 1) + R
        rb = lowmax.bit_length()
        if bd + rb > 64 or rb + span + ib > 64:
            continue
        exact = ps % (1 << bb) == 0
        bits1 = ((per - 1 if exact else per).bit_length() + rb) if cmp else 0
        return dict(sigma=sigma, n=n, s=s, R=R, K=s + R, rb=rb, bb=bb, bsh=48 - bb, cmul=(1 << 48) // ps, ps=ps,
                    per=per, ib=ib, cmp=cmp, bits1=bits1,
                    fast32=bits1 > K_SUB_BITS and bits1 - K_SUB_BITS <= K_LOW_MAX)
    return None


def _plan_pk8(p, np2=True):
    hb, sg = p["bb"] - 8, p["sigma"]
    if sg & (sg - 1):
        if not np2:
            return False
        return hb + ((p["per"] + 1) - 1).bit_length() + p["rb"] + p["ib"] <= 64
    lg = sg.bit_length() - 1
    return lg * p["s"] >= p["bb"] and hb + (lg * p["s"] - p["bb"]) + p["rb"] + p["ib"] <= 64


def _short_suffix_ties(dig, s, R, last=None):
    n, K = len(dig), s + R
    last = K - 1 if last is None else last
    seen = set()
    for L in range(1, min(last, n) + 1):
        x = tuple(int(v) for v in dig[n - L:n - L + K]) + (0,) * (K - min(K, L))
        if x in seen:
            return True
        seen.add(x)
    return False


def bucket_dmin(b, cmul, bsh):
    b = np.asarray(b, dtype=np.uint64)
    d0 = (b << np.uint64(bsh)) // np.uint64(cmul)
    return np.where(((d0 * np.uint64(cmul)) >> np.uint64(bsh)) == b, d0, d0 + np.uint64(1))


def _dense_digits(text):
    """(n, sigma, the text as dense digits 0 .. sigma - 1)."""
    t = np.ascontiguousarray(text, dtype=np.uint8)
    present = np.zeros(256, bool)
    present[np.unique(t)] = True
    return int(t.size), int(present.sum()), (np.cumsum(present) - 1)[t].astype(np.uint64)


def host_plan(sigma, n, tail, init_chars=0, eonly=False, bb=None, no_cmp=False):
    """The plan build_packed (sa_build.hip plan_round1) settles on with
    round1="bucketed": the compact layout, the original one when the text's
    tail ties (or debug no_cmp), the E-only one for a non-power-of-two
    alphabet that packs only without the end bit (or debug eonly).  tail: the
    text's last K_MAX_K dense digits.  None: no bucketed plan (round 1 is the
    LSD sort)."""
    K = init_chars if init_chars > 0 else min_chars(sigma, n)
    p = plan_bucketed(sigma, n, K, 0 if no_cmp else 1, bb)
    if p is None:
        return None
    if p["cmp"] and _short_suffix_ties(tail, p["s"], p["R"]):
        p = plan_bucketed(sigma, n, K, 0, bb)
        if p is None:
            return None
    np2 = (sigma & (sigma - 1)) != 0
    if p["cmp"] == 1 and (np2 or eonly):
        p2 = plan_bucketed(sigma, n, K, 2, bb)
        if ((eonly or not _plan_pk8(p)) and p2 is not None and (eonly or _plan_pk8(p2))
                and not _short_suffix_ties(tail, p2["s"], p2["R"], p2["K"])):
            p = p2
    return p


def text_plan(text, init_chars=0, eonly=False, bb=None, no_cmp=False):
    """host_plan of a text, with "pk8": whether plan_pk8 packs its first-pass
    items (one GPU, no debug no_pk8)."""
    n, sigma, dig = _dense_digits(text)
    p = host_plan(sigma, n, dig[-K_MAX_K:], init_chars, eonly, bb, no_cmp)
    return None if p is None else dict(p, pk8=_plan_pk8(p))


# --------------------------------------------------------------------------
# the window model
# --------------------------------------------------------------------------
class WindowModel:
    """The bucketed first round of `text` at init_chars (0: auto) on one GPU,
    forced (round1="bucketed") with debug fast32_small: the layout the host
    picks (compact, E-only with `eonly`, the original one when the text's tail
    ties), the windows and where k_window_split sends them.  bb: the bucket
    bits forced by debug bb17 / bb18."""

    def __init__(self, text, init_chars=0, eonly=False, bb=None):
        n, sigma, dig = _dense_digits(text)
        p = host_plan(sigma, n, dig[-K_MAX_K:], init_chars, eonly, bb)
        assert p is not None, (sigma, n, init_chars, bb)
        self.plan, self.n, self.sigma = p, n, sigma
        s, R, rb, sg = p["s"], p["R"], p["rb"], np.uint64(sigma)
        assert sigma ** R < 2 ** 62 and p["ps"] <= 2 ** 32
        pad = np.concatenate([dig, np.zeros(s + R, np.uint64)])   # digit 0 past the end
        D = np.zeros(n, np.uint64)
        for q in range(s):
            D = D * sg + pad[q:q + n]
        r = np.zeros(n, np.uint64)
        for q in range(s, s + R):
            r = r * sg + pad[q:q + n]
        L = np.uint64(n) - np.arange(n, dtype=np.uint64)
        if p["cmp"] == 2:
            low = r
        elif p["cmp"] == 1:
            low = np.uint64(2) * r + (L >= np.uint64(s + R)).astype(np.uint64)
        else:
            tl = np.minimum(np.where(L >= np.uint64(s), L - np.uint64(s), 0), np.uint64(R))
            low = np.where(L < np.uint64(s), L - np.uint64(1), np.uint64(s) + r * np.uint64(R + 1) + tl)
        assert int(low.max()) < (1 << rb)
        bucket = (D * np.uint64(p["cmul"])) >> np.uint64(p["bsh"])
        nb = 1 << p["bb"]
        rel = ((D - bucket_dmin(bucket, p["cmul"], p["bsh"])) << np.uint64(rb)) | low
        key1 = (D << np.uint64(rb)) | low
        self.bucket_sizes = np.bincount(bucket.astype(np.int64), minlength=nb)
        bstart = np.concatenate([[0], np.cumsum(self.bucket_sizes)]).astype(np.int64)   # bstart[nb] = n
        # k_window_starts_tab: wb[j] = lower_bound(bstart, j W) (nb past the end), ws[j] = bstart[wb[j]]
        nw = (n + K_WIN_STRIDE - 1) // K_WIN_STRIDE
        x = np.arange(nw + 1, dtype=np.int64) * K_WIN_STRIDE
        wb = np.where(x >= n, nb, np.searchsorted(bstart, x, side="left"))
        ws = bstart[wb]
        size = ws[1:] - ws[:-1]
        listed = size > 0
        one = listed & (wb[1:] - wb[:-1] == 1) & bool(p["fast32"])
        self.ws, self.wb = ws, wb
        self.listed = int(listed.sum())
        self.largest_window = int(size.max())
        self.one_windows = np.flatnonzero(one)
        self.one_buckets = wb[:-1][one]
        self.one_sizes = size[one]

        def runs(v):                       # sorted values -> each run's first index and length
            v = np.sort(v)
            first = np.ones(n, bool)
            first[1:] = v[1:] != v[:-1]
            at = np.flatnonzero(first)
            return v[at], np.diff(np.append(at, n))

        # tie groups of key1 (what round 1 leaves unsorted: U members, G groups)
        _, glen = runs(key1)
        self.distinct = len(glen)
        self.unsorted = int(glen[glen > 1].sum())
        self.groups = int((glen > 1).sum())
        self.largest_group = int(glen.max())
        self.dense = self.unsorted > n // K_SPARSE_DIV
        # largest sub-bucket (top kSubBits of the bits1-bit relative key) of every bucket
        self.bucket_maxsub = np.zeros(nb, np.int64)
        if p["fast32"]:
            sub = rel >> np.uint64(p["bits1"] - K_SUB_BITS)
            assert int(sub.max()) < (1 << K_SUB_BITS)
            cell, clen = runs((bucket << np.uint64(K_SUB_BITS)) | sub)
            np.maximum.at(self.bucket_maxsub, (cell >> np.uint64(K_SUB_BITS)).astype(np.int64), clen)
        self.one_maxsub = self.bucket_maxsub[self.one_buckets] if len(self.one_buckets) else np.zeros(0, np.int64)
        self.one_bucket_windows = int(one.sum())
        self.clustered = int((self.one_maxsub > K_MAX_SUB).sum())
        # k_window_split's retry list plus the windows k_bucket_sort adds to it
        self.retried = (self.listed - self.one_bucket_windows) + self.clustered if p["fast32"] else None

    def class_counts(self):
        return [int(((self.one_maxsub >= lo) & (self.one_maxsub <= hi)).sum()) for lo, hi in SUB_CLASSES]

    def summary(self):
        p = self.plan
        return dict(n=self.n, sigma=self.sigma, K=p["K"], s=p["s"], R=p["R"], cmp=p["cmp"], bits1=p["bits1"],
                    low_bits=p["bits1"] - K_SUB_BITS, listed=self.listed, one=self.one_bucket_windows,
                    classes=self.class_counts(), retried=self.retried, largest=self.largest_window,
                    unsorted=self.unsorted, groups=self.groups, largest_group=self.largest_group, dense=self.dense,
                    min_one=int(self.one_sizes.min()) if len(self.one_sizes) else 0,
                    max_one=int(self.one_sizes.max()) if len(self.one_sizes) else 0)


# --------------------------------------------------------------------------
# the generator
# --------------------------------------------------------------------------
class _Rng:
    """Counter-based splitmix64: the same stream on every numpy."""

    def __init__(self, seed):
        self.seed, self.at = np.uint64(seed), 0

    def u64(self, k):
        with np.errstate(over="ignore"):
            i = np.arange(self.at + 1, self.at + k + 1, dtype=np.uint64)
            z = self.seed + i * np.uint64(0x9E3779B97F4A7C15)
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        self.at += k
        return z ^ (z >> np.uint64(31))

    def below(self, k, m):
        """k values in [0, m); m a number or an array of k bounds."""
        return (((self.u64(k) >> np.uint64(32)) * np.asarray(m, dtype=np.uint64)) >> np.uint64(32)).astype(np.int64)

    def perm(self, k):
        return np.argsort(self.u64(k), kind="stable")


def _digits(v, sigma, k):
    """[len(v), k] base-sigma digits of v, most significant first."""
    v = np.asarray(v, dtype=np.int64)
    out = np.empty((len(v), k), np.int64)
    for q in range(k - 1, -1, -1):
        out[:, q] = v % sigma
        v = v // sigma
    return out


def anchored_text(kind, n, block, alen, buckets, anchor=1, skip=0, dense=False, seed=1):
    """The text described in the module docstring.  buckets: (count, T, lows)
    for consecutive usable buckets of the anchored D range after the first
    `skip` of them (usable: holds a D value whose digits obey the anchor
    rule); lows = 0 draws the bits below the sub-bucket at random, lows > 0
    from that many values.  n must be a multiple of block, block of alen.  The
    layout is the auto plan's at n with the compact low (the text ends in its
    largest symbol)."""
    alpha = np.frombuffer(ALPHABETS[kind], np.uint8)
    sigma, a = len(alpha), anchor
    assert n % block == 0 and block % alen == 0 and 0 < a < sigma - 1
    p = plan_bucketed(sigma, n, min_chars(sigma, n), 1)
    assert p and p["fast32"], p
    s, R, K, rb = p["s"], p["R"], p["K"], p["rb"]
    low_bits = p["bits1"] - K_SUB_BITS
    tb = low_bits - 1                      # bits of r below the sub-bucket (rel low = 2 r + 1)
    assert K <= block and alen < s and 1 <= low_bits <= rb
    rng = _Rng(seed)
    nblocks = n // block
    # columns that never hold the anchor symbol (any alen consecutive positions
    # past the anchor include one; a run cannot start before a block either)
    col = np.arange(block)
    no_a = ((col % alen == 0) & (col >= alen)) | (col == block - 1)

    def ok_digits(d, c0):                  # rows of digits at columns c0 ...
        return ~((d == a) & no_a[c0:c0 + d.shape[1]]).any(axis=1)

    # valid D values of the anchored range, by bucket
    per_anchor = sigma ** (s - alen)
    d_lo = sum(a * sigma ** q for q in range(s - alen, s))
    Dv = np.arange(d_lo, d_lo + per_anchor, dtype=np.int64)
    dd = _digits(Dv, sigma, s)
    Dv = Dv[ok_digits(dd[:, alen:], alen)]
    Db = ((Dv.astype(np.uint64) * np.uint64(p["cmul"])) >> np.uint64(p["bsh"])).astype(np.int64)
    usable = np.unique(Db)
    assert skip + len(buckets) <= len(usable), (skip, len(buckets), len(usable))
    # valid r values, grouped by the bits above tb
    rv = np.arange(sigma ** R, dtype=np.int64)
    rv = rv[ok_digits(_digits(rv, sigma, R), s)]
    rtop, rstart, rcount = np.unique(rv >> tb, return_index=True, return_counts=True)

    rows = []                              # anchored blocks' first K digits
    for i, (count, T, lows) in enumerate(buckets):
        if count == 0:
            continue
        b = usable[skip + i]
        Dc = Dv[Db == b]
        ncand = len(Dc) * len(rtop)
        assert 0 < T <= ncand, (i, T, ncand)
        cand = rng.perm(ncand)[:T]         # T distinct (D, r top) pairs: T distinct sub-buckets
        neck = cand[np.arange(count) % T]
        Dn, rt = Dc[neck // len(rtop)], neck % len(rtop)
        pick = rng.below(count, rcount[rt] if lows == 0 else np.minimum(rcount[rt], lows))
        rn = rv[rstart[rt] + pick]
        rows.append(np.concatenate([_digits(Dn, sigma, s), _digits(rn, sigma, R)], axis=1))
    rows = np.concatenate(rows)
    na = len(rows)
    assert na <= nblocks, (na, nblocks)

    def filler(shape, c0):                 # random digits, never a where no_a says so
        k = shape[0] * shape[1]
        v = rng.below(k, sigma - 1).reshape(shape)
        free = rng.below(k, sigma).reshape(shape)
        v = v + (v >= a)
        return np.where(no_a[c0:c0 + shape[1]][None, :], v, free)

    blocks = np.empty((nblocks, block), np.int64)
    blocks[:na, :K] = rows
    blocks[:na, K:] = filler((na, block - K), K)
    nf = nblocks - na                      # filler blocks: no a at column 0 either
    piece = 4 if dense else 1
    f = filler((nf, block), 0)
    f[:, 0] = np.where(f[:, 0] == a, a + 1, f[:, 0])
    npc = nf // piece
    if dense:                              # every piece of the first half again in the second
        half = npc // 2 * piece
        f[half:2 * half] = f[:half]
    blocks[na:] = f
    # shuffle: anchored blocks one by one, filler pieces whole
    ulen = np.concatenate([np.ones(na, np.int64), np.full(npc, piece, np.int64),
                           np.ones(nf - npc * piece, np.int64)])
    ustart = np.cumsum(ulen) - ulen
    o = rng.perm(len(ulen))
    ol = ulen[o]
    blocks = blocks[np.repeat(ustart[o] - (np.cumsum(ol) - ol), ol) + np.arange(nblocks)]
    text = alpha[blocks.reshape(-1)]
    text[-1] = alpha[-1]                   # no tail run of the smallest symbol: the compact layout
    return text


# --------------------------------------------------------------------------
# the texts the GPU tests use (tests/test_gpu_local_sort.py); their coverage
# is asserted on the CPU by tests/test_local_sort_texts.py
# --------------------------------------------------------------------------
# largest sub-bucket wanted, in turn: every class, both sides of each network
# size and of kMaxSub
WANT_MIXED = (3, 4, 7, 8, 11, 12, 15, 16, 17, 40, 64, 65, 90, 2, 6, 10, 14, 33)
# mostly small sub-buckets (few ties among the anchored suffixes: a sparse round 1)
WANT_SMALL = (2, 3, 4, 2, 5, 3, 8, 2, 9, 3, 12, 4, 13, 2, 16, 3, 17, 4, 64, 2, 65, 3, 80, 2, 3, 4)


def _class_cycle(k, base, seed, want=WANT_MIXED, lows=2):
    """k buckets of base .. base + 150 suffixes whose largest sub-bucket
    cycles through `want`; every 5th draws its low key bits from `lows`
    values only (large tie groups)."""
    out = []
    for i in range(k):
        c = base + (i * 37 + seed) % 151
        big = want[i % len(want)]
        T = -(-c // big)
        while -(-c // T) != big:           # ceil(c / T) == big exactly
            c += 1
            T = -(-c // big)
        out.append((c, T, lows if lows and i % 5 == 0 else 0))
    return out


def _dna_buckets(want, lows):
    b = _class_cycle(100, 1030, 0, want, lows)
    # a window within one wave-row of kBsCap; windows a few items on each side
    # of one and of two wave-rows, and exactly on them
    b += [(K_BS_CAP - 200, 1100, 0)]
    b += [(c, -(-c // 3), 0) for c in (K_WAVE_ROW - 3, K_WAVE_ROW, K_WAVE_ROW + 3, 2 * K_WAVE_ROW - 2,
                                       2 * K_WAVE_ROW + 5)]
    # windows under 64 items: a small bucket of t suffixes after one of g is a
    # one-bucket window when the last window boundary at or before its start
    # lies 1024 - t .. g - 1 before it; 19 pairs of 1020 + 60, which step that
    # distance by 56 = the range's width, pass through it whatever it starts at
    for i in range(19):
        b += [(1020, 340, 0), (60, 20, 0)]
    b += [(1100, 300, 0)]
    return b


DNA_N = 3 << 20


@functools.lru_cache(maxsize=None)
def text(name):
    if name == "dna_sparse":
        return anchored_text("dna", DNA_N, 16, 4, _dna_buckets(WANT_SMALL, 0), seed=11)
    if name == "dna_dense":
        return anchored_text("dna", DNA_N, 16, 4, _dna_buckets(WANT_MIXED, 2), dense=True, seed=12)
    if name == "byte256":
        return anchored_text("byte256", 1 << 21, 8, 1, _class_cycle(120, 1030, 3), skip=2, seed=13)
    if name == "alnum":
        return anchored_text("alnum", 1 << 21, 8, 1, _class_cycle(120, 1030, 5), skip=40, seed=14)
    raise KeyError(name)


def xq_text(n):
    """The dense DNA recipe at a size whose second pass can take per-XCD
    queues (blocks of 32 from 2^24: K = 17 symbols there)."""
    return anchored_text("dna", n, 16 if n < (1 << 24) else 32, 4, _dna_buckets(WANT_MIXED, 2), dense=True, seed=15)


TEXTS = ("dna_sparse", "dna_dense", "byte256", "alnum")
DNA_TEXTS = ("dna_sparse", "dna_dense")


@functools.lru_cache(maxsize=None)
def model(name, init_chars=0, eonly=False, bb=None):
    return WindowModel(text(name), init_chars, eonly, bb)


# --------------------------------------------------------------------------
# the second bucket pass (sa_split.h k_split_seg): its work units, and the
# texts of tests/test_gpu_second_pass.py; their coverage is asserted on the
# CPU by tests/test_second_pass_texts.py
# --------------------------------------------------------------------------
K_LO_BITS = 8           # sa_bucket.h kLoBits: the first pass's digit
K_SEGS = 1 << K_LO_BITS
K_XQ = 8                # per-XCD queues (sa_bucket.h kXq)
K_XQ_SLACK = 2048       # sa_split.h kXqSlack
UNIT_PK = 12 * 1024     # SA_ITEMS_PK x 1024 threads: packed 8-byte items
UNIT_B = 10 * 1024      # SA_ITEMS_B x 1024: 12-byte items


class SecondPassUnits:
    """What second_pass_units() returns:
    seg_sizes[256]      items of segment l = bucket & 255 (the pass's input order)
    digit_tot[2^hb]     items of high digit h = bucket >> 8
    count[2^hb, 256]    items of bucket (h, l)
    seg_units[256]      ceil(size / unit) units of segment l
    unit_seg[U]         the segment of unit u: units are numbered segment by
                        segment, empty segments take none (k_split_seg s_ubase)
    unit_size[U]        its items (a segment's last unit holds the rest)
    unit_queue[U]       u mod 8, the per-XCD queue that takes it
    owns[8, 256]        queue q takes at least one unit of segment l
    ub[8, 2^hb]         sum of count(h, l) over the segments q owns: an upper
                        bound of q's share of digit h, exact where every
                        segment is one unit
    cap[2^hb]           k_xq_dh's sub-region of one queue's digit h"""

    def __init__(self, bucket, bb, unit):
        hb = bb - K_LO_BITS
        self.bb, self.hb, self.unit = bb, hb, unit
        b = np.asarray(bucket, dtype=np.int64)
        assert int(b.max()) < (1 << bb)
        self.count = np.bincount(b, minlength=1 << bb).reshape(1 << hb, K_SEGS)
        self.seg_sizes = self.count.sum(axis=0)
        self.digit_tot = self.count.sum(axis=1)
        self.seg_units = -(-self.seg_sizes // unit)
        self.unit_seg = np.repeat(np.arange(K_SEGS), self.seg_units)
        first = np.cumsum(self.seg_units) - self.seg_units          # s_ubase
        within = np.arange(len(self.unit_seg)) - first[self.unit_seg]
        self.unit_size = np.minimum(self.seg_sizes[self.unit_seg] - within * unit, unit)
        self.unit_queue = np.arange(len(self.unit_seg)) % K_XQ
        self.owns = np.zeros((K_XQ, K_SEGS), bool)
        self.owns[self.unit_queue, self.unit_seg] = True
        self.ub = self.owns.astype(np.int64) @ self.count.T
        self.cap = self.digit_tot // K_XQ + self.digit_tot // 128 + K_XQ_SLACK

    @property
    def last_unit(self):
        """Items of each non-empty segment's last unit."""
        sz = self.seg_sizes[self.seg_sizes > 0]
        return sz - (-(-sz // self.unit) - 1) * self.unit

    def summary(self):
        sz = self.seg_sizes
        return dict(bb=self.bb, unit=self.unit, units=len(self.unit_seg), seg_min=int(sz.min()), seg_max=int(sz.max()),
                    empty_segs=int((sz == 0).sum()), empty_digits=int((self.digit_tot == 0).sum()),
                    two_unit=int((self.seg_units == 2).sum()),
                    short_last=int(((self.last_unit >= 1) & (self.last_unit <= 63)).sum()),
                    ub_over_cap=float((self.ub / self.cap).max()))


def second_pass_buckets(text, bb):
    """bucket = (D cmul) >> bsh of every suffix under the auto plan at `bb`
    bucket bits (D: the first s dense digits, digit 0 past the end; the bucket
    depends on s and cmul only, not on the key1 low's layout)."""
    n, sigma, dig = _dense_digits(text)
    p = host_plan(sigma, n, dig[-K_MAX_K:], bb=bb)
    assert p is not None and p["bb"] == bb, (sigma, n, bb, p)
    pad = np.concatenate([dig, np.zeros(p["s"], np.uint64)])
    D = np.zeros(n, np.uint64)
    for q in range(p["s"]):
        D = D * np.uint64(sigma) + pad[q:q + n]
    return (D * np.uint64(p["cmul"])) >> np.uint64(p["bsh"])


def second_pass_units(text, bb, unit):
    return SecondPassUnits(second_pass_buckets(text, bb), bb, unit)


SP_N = 3 << 20
# the TT-free text: at 3 x 2^20 nearly all of its 216 non-empty segments are
# two units (one full, one small), a queue owns a unit of ~52 of them, and the
# bound ub(q, h) passes the sub-region by 2 % at 16 bucket bits whatever the
# seed (0.24 tot(h) against tot(h) / 8 + tot(h) / 128 + 2048 at tot(h) ~ 18000);
# at 5 x 2^19 a quarter of the segments are two units and ub stays under 0.65
# of the capacity
SP_NO_TT_N = 5 << 19
SP_SMALL_N = 11 * 6144 + 5   # the smallest size class of the bucketed round (tests/test_gpu_first_pass.py)
SP_TEXTS = ("dna_uniform", "dna_no_tt", "dna_no_tt_small", "binary", "byte256", "alnum", "ascii127")
SP_XQ_DNA = ("dna_uniform", "dna_no_tt", "dna_no_tt_small")   # per-XCD queues in every mode
# init_chars of the per-XCD builds: the queues need the fixed-span local sort,
# whose key span must pass kSubBits bits; the small text's auto K = 13 leaves
# 9 .. 11, K = 16 gives 15 .. 17 (0: auto)
SP_XQ_CHARS = {"dna_no_tt_small": 16}
SP_XQ_OTHER = ("alnum", "byte256")                             # ... at 17 and 18 bucket bits
SP_BBS = (16, 17, 18)
SP_ROUNDS_N = 1_500_007


def _no_tt(t, seed):
    """Wherever TT occurs the second T is redrawn from ACG, until no TT is
    left (the draws: the same splitmix64 stream as the oracle's generator);
    the text keeps its last symbol T."""
    t = t.copy()
    t[-1] = ord("T")
    if t[-2] == ord("T"):
        t[-2] = ord("G")
    acg = np.frombuffer(b"ACG", np.uint8)
    rng = _Rng(seed)
    while True:
        at = np.flatnonzero((t[1:-1] == ord("T")) & (t[:-2] == ord("T"))) + 1
        if len(at) == 0:
            break
        t[at] = acg[rng.below(len(at), 3)]
    assert not ((t[1:] == ord("T")) & (t[:-1] == ord("T"))).any()
    return t


@functools.lru_cache(maxsize=None)
def sp_text(name):
    """The texts of tests/test_gpu_second_pass.py, from the oracle's generator;
    all end in their largest symbol (the compact layout)."""
    from oracle import oracle as O
    if name == "dna_uniform":
        t = O.gen_text("dna", SP_N, seed=101)
    elif name == "dna_no_tt":
        return _no_tt(O.gen_text("dna", SP_NO_TT_N, seed=102), 1102)
    elif name == "dna_no_tt_small":
        return _no_tt(O.gen_text("dna", SP_SMALL_N, seed=103), 1103)
    elif name == "binary":
        t = O.gen_text("binary", 1 << 20, seed=104)
    elif name == "byte256":
        t = O.gen_text("byte256", 1 << 21, seed=105)
    elif name in ("alnum", "ascii127"):
        t = O.gen_text(name, 1_500_007, seed=106 + len(name))
    elif name == "dna_rounds":
        # later rounds: 300 planted copies of 40-160 symbols keep members
        # after round 2 (the recipe of test_gpu_parity.py test_key1_round_two)
        t = O.gen_text("dna", SP_ROUNDS_N, seed=31)
        rng = _Rng(29)
        src, dst = rng.below(300, SP_ROUNDS_N - 200), rng.below(300, SP_ROUNDS_N - 200)
        for a, b, ln in zip(src, dst, 40 + rng.below(300, 120)):
            t[b:b + ln] = t[a:a + ln].copy()
    else:
        raise KeyError(name)
    t[-1] = t.max()
    return t


@functools.lru_cache(maxsize=None)
def sp_units(name, bb, unit=UNIT_PK):
    return second_pass_units(sp_text(name), bb, unit)


@functools.lru_cache(maxsize=None)
def sp_plan(name, bb=None, eonly=False, no_cmp=False, init_chars=0):
    return text_plan(sp_text(name), init_chars, eonly, bb, no_cmp)
