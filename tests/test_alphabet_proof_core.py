"""The host-compilable arithmetic of the sampled alphabet (hpc_suffix_array_amd/
csrc/sa_alpha.h): g++ builds tests/cpp/alphabet_check.cpp, which checks the
first bucket pass's DNA and byte-map predicates against byte-wise tests and the
sample's layout against its rules, once plainly and once with
-fsanitize=address,undefined as a stand-alone program.  Plus the two debug
names, the statistics field and the constants the kernels share with the
header.  No GPU needed."""
import ctypes
import os
import re
import subprocess

from hpc_suffix_array_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hpc_suffix_array_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "alphabet_check.cpp")


def _build_and_run(tmp_path, name, flags, timeout):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, SRC, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok "), out.stdout
    assert int(out.stdout.split()[1]) > 1_000_000, out.stdout


def test_predicates_match_bytewise_tests(tmp_path):
    _build_and_run(tmp_path, "alphabet_check", ["-O2"], 300)


def test_predicates_under_sanitizers(tmp_path):
    """The same program with AddressSanitizer and UBSan: a shift by a word's
    full width or an overflowing sum in the SWAR tests is reported."""
    _build_and_run(tmp_path, "alphabet_check_san",
                   ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], 600)


def test_debug_names_agree():
    hdr = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    flags = {m.group(1).lower(): int(m.group(2), 16)
             for m in re.finditer(r"^#define SA_DEBUG_(\w+)\s+(0x[0-9a-fA-F]+)u\b", hdr, re.M)}
    assert flags["no_alpha_sample"] == N.DEBUG_FLAGS["no_alpha_sample"] == 0x10000
    assert flags["alpha_sample_small"] == N.DEBUG_FLAGS["alpha_sample_small"] == 0x20000
    assert N.debug_bits(("no_alpha_sample", "alpha_sample_small")) == 0x30000
    assert flags == N.DEBUG_FLAGS


def test_stats_field_is_last_and_named():
    hdr = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    body = re.search(r"typedef struct \{(?:(?!typedef).)*?\} sa_stats;", hdr, re.S).group(0)
    assert re.search(r"int32_t alphabet;[^;]*\} sa_stats;", body, re.S), "alphabet is sa_stats' last field"
    assert N.SaStats._fields_[-1][0] == "alphabet"
    vals = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define SA_ALPHABET_(\w+) (\d+)", hdr)}
    assert vals == {"exact": 0, "sampled": 1, "refuted": 2}
    st = N.SaStats()
    for v, name in ((0, "exact"), (1, "sampled"), (2, "refuted")):
        st.alphabet = v
        assert st.to_dict()["alphabet"] == name
    assert ctypes.sizeof(N.SaStats) % 8 == 0


def test_sample_constants():
    """The sample reads whole 4 KiB blocks, one of every 64: at most n / 64
    bytes; the sample kernel covers a block with one 16-byte chunk per lane."""
    src = open(os.path.join(CSRC, "sa_alpha.h")).read()
    assert int(re.search(r"kAlphaBlock\s*=\s*(\d+)", src).group(1)) == 4096
    assert int(re.search(r"kAlphaEvery\s*=\s*(\d+)", src).group(1)) == 64
    kern = open(os.path.join(CSRC, "sa_kernels.h")).read()
    assert "kBlock * 16 == (int)kAlphaBlock" in kern
