"""The debug flags of sa_opts.debug: every Python name (_native.DEBUG_FLAGS)
maps to the bit of its SA_DEBUG_* constant in include/sa_hip.h and back, the
bits are distinct single bits, and ls_one_wg -- the one-workgroup launch of
the fixed-span local sort (tests/test_gpu_local_sort_handover.py) -- is one
of them.  No GPU needed."""
import os
import re

import pytest

from hpc_suffix_array_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_flags():
    hdr = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    return {m.group(1).lower(): int(m.group(2), 16)
            for m in re.finditer(r"^#define SA_DEBUG_(\w+)\s+(0x[0-9a-fA-F]+)u\b", hdr, re.M)}


def test_names_match_header():
    assert N.DEBUG_FLAGS == _header_flags()


def test_single_distinct_bits():
    bits = sorted(N.DEBUG_FLAGS.values())
    assert all(b and b & (b - 1) == 0 for b in bits), bits
    assert len(set(bits)) == len(bits)
    assert max(bits) < 1 << 32     # sa_opts.debug is a uint32_t


def test_ls_one_wg():
    assert _header_flags()["ls_one_wg"] == 0x8000
    assert N.debug_bits(("ls_one_wg",)) == 0x8000
    assert N.debug_bits(("fast32_small", "ls_one_wg")) == 0x2000 | 0x8000
    with pytest.raises(ValueError):
        N.debug_bits(("ls_one_workgroup",))


def test_opts_struct_unchanged():
    """The flag is a bit of an existing field: sa_opts keeps its layout."""
    import ctypes
    assert ctypes.sizeof(N.SaOpts) == 32
    assert N.SaOpts.debug.offset == 20 and N.SaOpts.debug.size == 4
