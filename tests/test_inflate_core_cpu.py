"""csrc/gki_inflate_core.h as a host program under AddressSanitizer and UndefinedBehaviorSanitizer: every good vector of
tests/bgzf_cases.py inflates to what zlib compressed, every malformed one ends with its status, and 2 000 seeded
corruptions of the good ones all end with a status, inside their buffers, with nothing for the sanitizers to report.
The program (tests/inflate_core_main.cpp) has its own main and is built here with the system's C++ compiler, or with
hipcc's host side; malformed input is tried in bulk here, on the CPU, and nowhere on a device."""
import os
import shutil
import struct
import subprocess
import zlib

import pytest

import bgzf_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "inflate_core_main.cpp")
HIPCC = "/opt/rocm/bin/hipcc"
SANITIZE = "-fsanitize=address,undefined"


def _compilers():
    for name in ("c++", "g++", "clang++"):
        path = shutil.which(name)
        if path:
            yield [path, "-O1", "-g", "-std=c++17", SANITIZE, "-fno-sanitize-recover=undefined"]
    if os.path.exists(HIPCC):
        yield [HIPCC, "-x", "c++", "-O1", "-g", "-std=c++17", "-Xarch_host", SANITIZE]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """The program, built by the first compiler that can build anything with the sanitizers (tried on an empty main).
    Skipped only when there is no such compiler; the program itself failing to build fails the tests."""
    tmp = tmp_path_factory.mktemp("inflate_core")
    probe = str(tmp / "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    for cmd in _compilers():
        built = subprocess.run(cmd + [probe, "-o", str(tmp / "probe")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        if built.returncode == 0 and subprocess.run([str(tmp / "probe")]).returncode == 0:
            break
    else:
        pytest.skip("no C++ compiler here that builds and runs a program with %s" % SANITIZE)
    out = str(tmp / "inflate_core_main")
    built = subprocess.run(cmd + [MAIN, "-o", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert built.returncode == 0, built.stdout.decode("utf-8", "replace")[-4000:]
    return out


def run(program, tmp_path, vectors):
    """[(status, bytes written, CRC-32 of them)] of (payload, crc, isize) vectors; the sanitizers must stay silent."""
    path = str(tmp_path / "vectors.bin")
    with open(path, "wb") as f:
        for payload, crc, isize in vectors:
            f.write(struct.pack("<III", len(payload), isize, crc) + payload)
    r = subprocess.run([program, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and r.stderr == b"", r.stderr.decode("utf-8", "replace")[-2000:]
    lines = r.stdout.decode().split("\n")[:-1]
    assert len(lines) == len(vectors)
    return [(int(a), int(b), int(c, 16)) for a, b, c in (line.split() for line in lines)]


def test_good_vectors_inflate_to_what_zlib_compressed(program, tmp_path):
    members = [(name, m) for name in sorted(cases.GOOD) for m in cases.GOOD[name]]
    got = run(program, tmp_path, [m[:3] for _, m in members])
    for (name, m), (status, n_out, crc) in zip(members, got):
        assert zlib.decompress(m[0], -15) == m[3], name                       # the vector itself, by zlib
        assert (status, n_out, crc) == (cases.OK, len(m[3]), zlib.crc32(m[3])), name


def test_malformed_vectors_end_with_their_status(program, tmp_path):
    names = sorted(cases.MALFORMED)
    got = run(program, tmp_path, [cases.MALFORMED[name][0][:3] for name in names])
    for name, (status, n_out, _) in zip(names, got):
        want = cases.MALFORMED[name][1]
        assert status == want, (name, status)
        assert n_out <= cases.MALFORMED[name][0][2]
    assert set(cases.GPU_MALFORMED) <= set(names)
    assert {want for _, want in cases.MALFORMED.values()} == set(range(1, 14))   # every status the core has


def test_fuzz_of_2000_corruptions_always_ends_with_a_status(program, tmp_path):
    vectors = list(cases.fuzz_cases(2000, 1234))
    got = run(program, tmp_path, vectors)
    failures = 0
    for (payload, crc, isize), (status, n_out, out_crc) in zip(vectors, got):
        assert 0 <= status <= 13 and 0 <= n_out <= isize
        if status == cases.OK:                           # a flip in padding bits: the output is still the original
            assert n_out == isize and out_crc == crc
        else:
            failures += 1
    assert failures > 1500
