"""Helpers shared by the tests of one long-lived context
(tests/test_gpu_streams_core.py, tests/test_gpu_call_sequences.py and the
child process of its epoch test).  TEST INFRASTRUCTURE ONLY: CPU references
and one build-and-compare step; nothing here decides what a test asserts."""
import numpy as np

PERIOD = b"abaababa"


def numpy_inverse(p):
    """The inverse permutation, uint32."""
    inv = np.empty(p.size, np.uint32)
    inv[p] = np.arange(p.size, dtype=np.uint32)
    return inv


def periodic(n):
    """n bytes of the period-8 text: most suffixes stay unsorted for many rounds."""
    return np.tile(np.frombuffer(PERIOD, np.uint8), n // len(PERIOD) + 1)[:n].copy()


def sort_reference(keys, bits):
    """torch's stable sort of the low `bits` bits of int64 keys, taken as
    unsigned: the permutation.  (64 bits: the sign bit flipped orders int64
    as uint64.)"""
    import torch
    masked = keys ^ torch.iinfo(torch.int64).min if bits == 64 else keys & ((1 << bits) - 1)
    return torch.sort(masked, stable=True)[1]


_sa = {}


def want_sa(oracle, t):
    """The oracle's SA of t, computed once per text."""
    key = t.tobytes()
    if key not in _sa:
        _sa[key] = oracle.sa_c(t)
    return _sa[key]


def build_ok(b, oracle, t, **kw):
    """Build t's SA on context b into a poisoned output and compare it with
    the oracle's; returns the statistics."""
    import torch
    t = np.ascontiguousarray(t)
    n = int(t.size)
    d_text = torch.from_numpy(t.copy()).cuda()
    d_sa = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    st = b.build(d_text, n, d_sa, **kw)
    torch.cuda.synchronize()
    assert (d_sa.cpu().numpy().view(np.uint32) == want_sa(oracle, t)).all(), (n, kw)
    return st
