"""The striped level 1 of the coalesced permutations (sa_check.h k_chk_bin /
k_chk_split / k_chk_cursors with eight stripes per bin) and its overflow
rerun, in the checker, in LCP's PHI / ISA + 1 / PLCP placements and in the
inverse suffix array.

Stripes are taken only by a call of at least 2^24 on a context whose keys[0]
holds the stripe regions, which a context sized for that call never does
(tests/perm_stripes_model.py, asserted on the CPU by
tests/test_perm_stripes_model.py), so every test here runs n = 2^24 (or
2^24 + 5) on one DeviceBuilder(1 << 26) and asserts with the model, before it
calls the library, that its input takes the path it is meant to take.  The
model only chooses inputs; the references are the oracle's adjacent-pair check
(oracle.check_c), numpy's inverse permutation and the closed-form SA / LCP of
the periodic text bytes(range(256)) * 65536, whose SA sends every bin's pairs
to one stripe (all 256 bins overflow in pass A, PHI and ISA + 1).

Everything stays on the device: corruptions are torch index operations on a
clone of the SA.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import perm_stripes_model as M   # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N24 = 1 << 24
CAP26 = 1 << 26
REPS = 1 << 16


@pytest.fixture(scope="module")
def b26(gpu):
    from hpc_suffix_array_amd import DeviceBuilder
    b = DeviceBuilder(CAP26)
    yield b
    b.close()


@pytest.fixture(scope="module")
def b24(gpu):
    from hpc_suffix_array_amd import DeviceBuilder
    b = DeviceBuilder(N24)
    yield b
    b.close()


def numpy_inverse(p):
    inv = np.empty(p.size, np.uint32)
    inv[p] = np.arange(p.size, dtype=np.uint32)
    return inv


_dna = {}


def dna(b26, oracle, n):
    """Random DNA of n bytes and its SA, built on the device once per n and
    confirmed once by the oracle's adjacent-pair check; plus the text with one
    byte changed and the oracle's verdict on the unchanged SA against it."""
    import torch
    if n not in _dna:
        d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
        d_sa = torch.empty(n, dtype=torch.int32, device="cuda")
        b26.generate_text(d_text, n, b"ACGT", seed=n)
        b26.build(d_text, n, d_sa)
        torch.cuda.synchronize()
        text = d_text.cpu().numpy()
        sa = d_sa.cpu().numpy().view(np.uint32)
        assert oracle.check_c(text, sa)
        p = n // 2
        changed = text.copy()
        changed[p] = ord("C") if text[p] != ord("C") else ord("G")
        d_changed = d_text.clone()
        d_changed[p] = int(changed[p])
        _dna[n] = dict(n=n, d_text=d_text, d_sa=d_sa, text=text, sa=sa, isa=numpy_inverse(sa), d_changed=d_changed,
                       changed_ok=oracle.check_c(changed, sa))
    return _dna[n]


def swap(d_sa, i, j):
    bad = d_sa.clone()
    bad[i], bad[j] = d_sa[j], d_sa[i]
    return bad


def put(d_sa, i, value):
    bad = d_sa.clone()
    bad[i] = value
    return bad


def corruptions(data, s1):
    """(name, corrupted SA on the device, expected verdict) of the matrix;
    s1: the level-1 bin bits of the plan under test."""
    import torch
    n, d_sa, sa, text = data["n"], data["d_sa"], data["sa"], data["text"]
    swaps = {"swap_first": (0, 1), "swap_last": (n - 2, n - 1),
             "swap_subbin_b_and_stripe": (8191, 8192),       # pass B sub-bin; tiles 0 / 1: stripes 0 / 1
             "swap_subbin_a": (16383, 16384),
             "swap_bin": ((1 << s1) - 1, 1 << s1),
             "swap_last_bin": ((((n - 1) >> s1) << s1) - 1, ((n - 1) >> s1) << s1)}
    for name, (i, j) in swaps.items():
        yield name, swap(d_sa, i, j), False
    i, j = 1000, 1000 + (1 << 21)
    assert text[sa[i]] == text[sa[j]] and sa[i] != sa[j]
    yield "swap_far_same_first_byte", swap(d_sa, i, j), False
    yield "duplicate_far", put(d_sa, n // 3, int(sa[2 * n // 3])), False
    yield "duplicate_adjacent", put(d_sa, 8192, int(sa[8191])), False
    yield "entry_n", put(d_sa, n // 5, n), False
    yield "entry_all_ones", put(d_sa, n - 1, -1), False
    yield "reversed", torch.flip(d_sa, [0]), False
    rng = np.random.default_rng(n)
    k = int(rng.integers(0, n - 32))
    perm = torch.from_numpy(rng.permutation(32)).cuda()
    sh = d_sa.clone()
    sh[k:k + 32] = d_sa[k:k + 32][perm]
    yield "local_shuffle", sh, bool(torch.equal(sh, d_sa))


_verdicts = {}


def matrix(b, cap, data, s1):
    """The verdict of b.check on every case of the matrix, each asserted
    against its expected value, the valid SA checked again after every False
    (no cursor or error word may leak into the next call)."""
    import torch
    key = (cap, data["n"])
    if key in _verdicts:
        return _verdicts[key]
    n, d_text, d_sa = data["n"], data["d_text"], data["d_sa"]
    torch.cuda.synchronize()
    out = {"valid": b.check(d_text, n, d_sa)}
    assert out["valid"] is True
    for name, bad, want in corruptions(data, s1):
        if not want:
            assert not torch.equal(bad, d_sa), name      # not a no-op
        torch.cuda.synchronize()
        out[name] = b.check(d_text, n, bad)
        assert out[name] == want, name
        if not out[name]:
            assert b.check(d_text, n, d_sa), f"valid SA after {name}"
    out["text_changed"] = b.check(data["d_changed"], n, d_sa)
    assert out["text_changed"] == data["changed_ok"]
    assert b.check(d_text, n, d_sa), "valid SA after text_changed"
    _verdicts[key] = out
    return out


@pytest.mark.parametrize("n", [N24, N24 + 5])
def test_checker_verdicts_striped(b26, oracle, n):
    pa, pb = M.plan_check(n, M.SUB_A), M.plan_check(n, M.SUB_B)
    assert M.plan_stripes(CAP26, n, pa).st == 8 and M.plan_stripes(CAP26, n, pb).st == 8
    assert pa.s1 == pb.s1
    matrix(b26, CAP26, dna(b26, oracle, n), pa.s1)


def test_checker_verdicts_unstriped_agree(b26, b24, oracle):
    n = N24
    assert not M.is_striped(N24, n, M.SUB_A) and not M.is_striped(N24, n, M.SUB_B)
    s1 = M.plan_check(n).s1
    data = dna(b26, oracle, n)
    striped = matrix(b26, CAP26, data, s1)
    plain = matrix(b24, N24, data, s1)
    assert striped.keys() == plain.keys()
    for name in striped:
        assert striped[name] == plain[name], name


@pytest.mark.parametrize("v", [1, 2, 3])
def test_checker_ab_shapes_striped(b26, oracle, v):
    """tune bits 20-23: 1 / 2 = 1024 / 512 level-1 bins (k_chk_bin with 7
    items per lane), 3 = the persistent split (k_split_p) over stripe regions."""
    import torch
    n = N24
    b1 = {1: 10, 2: 9, 3: 8}[v]
    pa, pb = M.plan_check(n, M.SUB_A, b1), M.plan_check(n, M.SUB_B, b1)
    assert M.plan_stripes(CAP26, n, pa).st == 8 and M.plan_stripes(CAP26, n, pb).st == 8
    data = dna(b26, oracle, n)
    d_text, d_sa, sa = data["d_text"], data["d_sa"], data["sa"]
    cases = {"swap_subbin": swap(d_sa, 8191, 8192),
             "swap_bin": swap(d_sa, (1 << pa.s1) - 1, 1 << pa.s1),
             "duplicate": put(d_sa, n // 3, int(sa[2 * n // 3])),
             "entry_n": put(d_sa, n // 5, n)}
    torch.cuda.synchronize()
    b26.set_debug(tune=v << 20)        # after the build: sa_build_device applies its own options
    try:
        assert b26.check(d_text, n, d_sa)
        for name, bad in cases.items():
            assert not torch.equal(bad, d_sa), name
            assert not b26.check(d_text, n, bad), name
            assert b26.check(d_text, n, d_sa), f"valid SA after {name}"
        # the persistent split serves every permutation: the inverse's values under it
        d_isa = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        b26.inverse(n, d_sa, d_isa)
        assert (d_isa.cpu().numpy().view(np.uint32) == data["isa"]).all()
    finally:
        b26.set_debug()
    assert b26.check(d_text, n, d_sa)


def test_striped_values_random_dna(b26, oracle):
    """No stripe overflows: the values LCP's PHI / ISA + 1 / PLCP placements
    and the inverse leave come from the striped kernels themselves (the last
    bin holds 5 entries), against the oracle's Kasai LCP and numpy's inverse."""
    import torch
    n = N24 + 5
    data = dna(b26, oracle, n)
    d_text, d_sa, text, sa = data["d_text"], data["d_sa"], data["text"], data["sa"]
    plan = M.plan_check(n)
    bs = M.plan_stripes(CAP26, n, plan)
    isa = data["isa"]
    assert bs.st == 8 and plan.nb1 == 129
    assert M.region_fill(sa, plan).max() < bs.scap and M.region_fill(isa, plan).max() < bs.scap
    d_out = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    b26.inverse(n, d_sa, d_out)
    assert (d_out.cpu().numpy().view(np.uint32) == isa).all()
    ref = oracle.lcp_c(text, sa)
    ln, pos = b26.lcp(d_text, n, d_sa, d_out)
    assert (d_out.cpu().numpy().view(np.uint32) == ref).all()
    assert bytes(text[pos:pos + ln]) == oracle.lrs_c(text, sa, ref)


@pytest.fixture(scope="module")
def periodic(gpu):
    """bytes(range(256)) * 65536 and its closed-form SA, made on the device."""
    import torch
    d_text = torch.arange(256, dtype=torch.int32, device="cuda").to(torch.uint8).repeat(REPS)
    r = torch.arange(N24, dtype=torch.int64, device="cuda")
    d_sa = ((r >> 16) + 256 * (REPS - 1 - (r & (REPS - 1)))).to(torch.int32)
    torch.cuda.synchronize()
    return d_text, d_sa


def assert_periodic_overflows():
    p = M.plan_check(N24)
    bs = M.plan_stripes(CAP26, N24, p)
    assert bs.st == 8
    # bin b of pass A / PHI / ISA + 1 takes the ranks k = (255 - b) 256 .. + 255 of every symbol
    # group: 256 tiles, all with the same tile index mod 8 (tests/test_perm_stripes_model.py
    # counts the whole array)
    stripe = ((np.arange(REPS) // M.TILE) % 8).reshape(256, 256)     # [255 - b][k mod 256]; 65536 c adds 8 c tiles
    assert (stripe == stripe[:, :1]).all()
    assert REPS > bs.scap


def test_overflow_rerun_checker(b26, periodic):
    """Every bin overflows its stripe in pass A: bit 128, then the whole check
    again with one stripe.  The verdicts follow from the construction (adjacent
    suffixes share up to 2^24 bytes: no adjacent-pair oracle here)."""
    assert_periodic_overflows()
    d_text, d_sa = periodic
    n = N24
    assert b26.check(d_text, n, d_sa)
    inside = 5 * REPS + 100                       # two suffixes of symbol 5, the longer first
    for name, bad in (("swap_inside_group", swap(d_sa, inside, inside + 1)),
                      ("swap_across_groups", swap(d_sa, REPS - 1, REPS)),
                      ("duplicate", put(d_sa, 3 * REPS + 7, int(d_sa[200 * REPS + 9])))):
        assert not b26.check(d_text, n, bad), name
        assert b26.check(d_text, n, d_sa), f"valid SA after {name}"


def test_overflow_rerun_inverse(b26, periodic):
    import torch
    assert_periodic_overflows()
    _, d_sa = periodic
    d_isa = torch.empty(N24, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    b26.inverse(N24, d_sa, d_isa)
    assert (d_isa.cpu().numpy().view(np.uint32) == numpy_inverse(M.periodic_sa(REPS))).all()


def test_overflow_rerun_lcp(b26, periodic):
    import torch
    assert_periodic_overflows()
    d_text, d_sa = periodic
    d_lcp = torch.empty(N24, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ln, pos = b26.lcp(d_text, N24, d_sa, d_lcp)
    assert (d_lcp.cpu().numpy().view(np.uint32) == M.periodic_lcp(REPS)).all()
    assert (ln, pos) == (256 * (REPS - 1), 0)


@pytest.mark.parametrize("k", [2048, 2049])
def test_inverse_at_the_stripe_capacity(b26, k):
    """Regions (bin 0, stripe 0) and (bin 1, stripe 1) filled to 8192 + k of
    10,240 slots: exactly full, and one pair too many (the rerun)."""
    import torch
    p = M.swapped_identity(N24, k)
    plan = M.plan_check(N24)
    f = M.region_fill(p, plan)
    scap = M.plan_stripes(CAP26, N24, plan).scap
    assert f.max() == f[0, 0] == f[1, 1] == 8192 + k and (f.max() > scap) == (k == 2049)
    d_p = torch.arange(N24, dtype=torch.int32, device="cuda")
    d_p[1 << 16:(1 << 16) + k] = torch.arange(1 << 13, (1 << 13) + k, dtype=torch.int32, device="cuda")
    d_p[1 << 13:(1 << 13) + k] = torch.arange(1 << 16, (1 << 16) + k, dtype=torch.int32, device="cuda")
    assert (d_p.cpu().numpy().view(np.uint32) == p).all()
    d_inv = torch.full((N24,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    b26.inverse(N24, d_p, d_inv)
    assert (d_inv.cpu().numpy().view(np.uint32) == numpy_inverse(p)).all()


def test_inverse_rejects_a_duplicate_then_recovers(b26):
    import torch
    from hpc_suffix_array_amd import SAError
    rng = np.random.default_rng(5)
    p = rng.permutation(N24).astype(np.uint32)
    assert M.region_fill(p, M.plan_check(N24)).max() < M.plan_stripes(CAP26, N24, M.plan_check(N24)).scap
    d_p = torch.from_numpy(p.view(np.int32)).cuda()
    d_bad = d_p.clone()
    d_bad[12345] = d_p[9_000_000]
    d_inv = torch.empty(N24, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(SAError):
        b26.inverse(N24, d_bad, d_inv)
    b26.inverse(N24, d_p, d_inv)
    assert (d_inv.cpu().numpy().view(np.uint32) == numpy_inverse(p)).all()


# --- the path, read from the library's trace -------------------------------
CHILD = r"""
import sys
import torch
from hpc_suffix_array_amd import DeviceBuilder

def mark(s):
    print("## " + s, file=sys.stderr, flush=True)

n, reps = 1 << 24, 1 << 16
b = DeviceBuilder(1 << 26)
d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
d_sa = torch.empty(n, dtype=torch.int32, device="cuda")
b.generate_text(d_text, n, b"ACGT", seed=7)
b.build(d_text, n, d_sa)
torch.cuda.synchronize()
mark("check random")
assert b.check(d_text, n, d_sa)
p_text = torch.arange(256, dtype=torch.int32, device="cuda").to(torch.uint8).repeat(reps)
r = torch.arange(n, dtype=torch.int64, device="cuda")
p_sa = ((r >> 16) + 256 * (reps - 1 - (r & (reps - 1)))).to(torch.int32)
torch.cuda.synchronize()
mark("check periodic")
assert b.check(p_text, n, p_sa)
out = torch.empty(n, dtype=torch.int32, device="cuda")
for k in (2048, 2049):
    p = torch.arange(n, dtype=torch.int32, device="cuda")
    p[1 << 16:(1 << 16) + k] = torch.arange(1 << 13, (1 << 13) + k, dtype=torch.int32, device="cuda")
    p[1 << 13:(1 << 13) + k] = torch.arange(1 << 16, (1 << 16) + k, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    mark("inverse %d" % k)
    b.inverse(n, p, out)
mark("lcp periodic")
b.lcp(p_text, n, p_sa, out)
mark("lcp random")
b.lcp(d_text, n, d_sa, out)
mark("small context")
s = DeviceBuilder(1 << 24)
assert s.check(d_text, n, d_sa)
mark("end")
s.close()
b.close()
print("child ok")
"""

TRACE = re.compile(r"^\[sa\] (check|inverse|lcp PHI|lcp ISA|lcp PLCP) \((\d+) stripes asked, (\d+)(?: / (\d+))? run"
                   r"[^)]*\)(?:: error bits (\S+))?$")


def parse_trace(stderr):
    """{section: [(what, asked, ran (pass A), ran (pass B) or None, error word or None)]}"""
    out, cur = {}, None
    for line in stderr.splitlines():
        if line.startswith("## "):
            cur = out.setdefault(line[3:], [])
            continue
        m = TRACE.match(line)
        if m and cur is not None:
            cur.append((m.group(1), int(m.group(2)), int(m.group(3)), None if m.group(4) is None else int(m.group(4)),
                        None if m.group(5) is None else int(m.group(5), 16)))
    return out


def test_paths_taken_by_the_trace(gpu):
    """One fresh process with SA_TRACE=1: the stripes each call really ran
    with, and which calls ran again with one stripe."""
    env = dict(os.environ, SA_TRACE="1")
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stderr[-4000:]
    t = parse_trace(r.stderr)
    assert t["check random"] == [("check", 8, 8, 8, 0)]
    first, second = t["check periodic"]
    assert first[:4] == ("check", 8, 8, 8) and first[4] & 0x80
    assert second == ("check", 1, 1, 1, 0)
    assert t["inverse 2048"] == [("inverse", 8, 8, None, 0)]
    first, second = t["inverse 2049"]
    assert first[:4] == ("inverse", 8, 8, None) and first[4] & 0x80
    assert second == ("inverse", 1, 1, None, 0)
    lcp = t["lcp periodic"]
    assert [x[:3] for x in lcp] == [("lcp PHI", 8, 8), ("lcp PHI", 1, 1), ("lcp ISA", 8, 8), ("lcp ISA", 1, 1),
                                    ("lcp PLCP", 8, 8)]
    assert lcp[0][4] & 0x80 and lcp[2][4] & 0x80 and not lcp[4][4] & 0x80
    assert lcp[1][4] is None and lcp[3][4] is None          # the last attempt is not read back
    lcp = t["lcp random"]
    assert [x[:3] for x in lcp] == [("lcp PHI", 8, 8), ("lcp ISA", 8, 8), ("lcp PLCP", 8, 8)]
    assert not any(x[4] & 0x80 for x in lcp)
    assert t["small context"] == [("check", 8, 1, 1, 0)]
