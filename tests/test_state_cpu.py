"""Checkpoints without a GPU: the host checksum against its numpy restatement, sph_state_peek against the pure-Python parser and
against damaged blobs, and the blob parser of csrc/sph_state.h as a stand-alone program under AddressSanitizer and UBSan."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG_NAME, ROOT, small_scene
import state_ref as S

CSRC = os.path.join(ROOT, PKG_NAME, "csrc")


@pytest.fixture(scope="module")
def scene(pkg):
    rec, sp = small_scene(pkg, n=300, grid=8, seed=5)
    return rec, sp


# ---- the checksum -------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", [0, 8, 16, 504, 512, 520, 80 * 4097])
def test_checksum_equals_numpy(pkg, nbytes):
    buf = np.random.default_rng(nbytes).integers(0, 256, nbytes, dtype=np.uint8)
    assert pkg.state_checksum_host(buf) == S.checksum(buf)


def test_checksum_refuses_odd_sizes(pkg):
    with pytest.raises(pkg.SphError, match="multiple of 8"):
        pkg.state_checksum_host(np.zeros(12, np.uint8))


def test_any_bit_flip_changes_both_lanes(pkg):
    buf = np.random.default_rng(1).integers(0, 256, 64, dtype=np.uint8)
    lo, hi = pkg.state_checksum_host(buf)
    for bit in range(64 * 8):
        b = buf.copy()
        b[bit // 8] ^= np.uint8(1 << (bit % 8))
        lo2, hi2 = pkg.state_checksum_host(b)
        assert lo2 != lo and hi2 != hi, bit


def test_swapping_two_records_changes_both_lanes(pkg, scene):
    rec = scene[0].copy()
    lo, hi = pkg.state_checksum_host(rec)
    assert rec[3].tobytes() != rec[200].tobytes()
    rec[[3, 200]] = rec[[200, 3]]
    lo2, hi2 = pkg.state_checksum_host(rec)
    assert lo2 != lo and hi2 != hi


def test_checksum_is_additive_over_pieces(pkg):
    buf = np.random.default_rng(2).integers(0, 256, 4096, dtype=np.uint8)
    whole = pkg.state_checksum_host(buf)
    for cut in (0, 8, 1000, 4088, 4096):
        assert S.add(S.checksum(buf[:cut]), S.checksum(buf[cut:], base=cut // 8)) == whole == S.checksum(buf)


# ---- peek -----------------------------------------------------------------------------------------------
def test_peek_agrees_with_the_python_parser(pkg, scene):
    rec, sp = scene
    for records in (rec, rec[:1], rec[:257]):
        blob = S.build_blob(pkg, records, sp)
        a, b = pkg.state_info(blob), pkg.state_sections(blob)
        assert bytes(a.pop("params")) == bytes(b.pop("params")) == bytes(sp)
        assert a == b
        assert a["n"] == len(records) and a["totalBytes"] == len(blob) and set(a["sections"]) == {"core", "particles"}
        assert a["sections"]["particles"]["sum"] == S.checksum(records.tobytes()) and a["sections"]["particles"]["bytes"] == 80 * len(records)
        assert a["sections"]["core"]["offset"] == S.align16(256 + 2 * 40) and a["sections"]["core"]["bytes"] == 280


def test_peek_refuses_damaged_blobs(pkg, scene):
    good, damaged = S.damaged_blobs(pkg, *scene)
    pkg.state_info(good)
    assert len(damaged) >= 9
    for name, blob, word in damaged:
        with pytest.raises(pkg.SphError, match="error -1:.*" + word):
            pkg.state_info(blob)
    for at in (41, 47, 200, 250, 300, 340, 700, len(good) - 1):          # a byte of the header, its reserve, its sum, the table, the payloads
        b = good.copy()
        b[at] ^= 1
        with pytest.raises(pkg.SphError):
            pkg.state_info(b)


# ---- the parser under sanitizers ------------------------------------------------------------------------
FUZZ_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "sph_state.h"
static unsigned long long rng_state = 88172645463325252ull;
static unsigned long long rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
// every checksum of a blob recomputed by hand, without the parser's bookkeeping
static bool sums_hold(const std::vector<unsigned char>& b) {
    sph::StateHeader h;
    if (b.size() < sizeof(h)) return false;
    memcpy(&h, b.data(), sizeof(h));
    const size_t table = sizeof(sph::StateEntry) * (size_t)h.sectionCount;
    if (h.sectionCount > 8 || b.size() < sizeof(h) + table) return false;
    uint64_t s[2] = {0, 0};
    sph::state_checksum(b.data(), 240, 0, s);
    sph::state_checksum(b.data() + sizeof(h), table, 30, s);
    if (s[0] != h.sum[0] || s[1] != h.sum[1]) return false;
    for (uint32_t i = 0; i < h.sectionCount; ++i) {
        sph::StateEntry e;
        memcpy(&e, b.data() + sizeof(h) + sizeof(e) * i, sizeof(e));
        if (e.offset > b.size() || e.bytes > b.size() - e.offset) return false;
        uint64_t c[2] = {0, 0};
        sph::state_checksum(b.data() + e.offset, (size_t)e.bytes, 0, c);
        if (c[0] != e.sum[0] || c[1] != e.sum[1]) return false;
    }
    return true;
}
int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<unsigned char> good;
    unsigned char buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) good.insert(good.end(), buf, buf + got);
    fclose(f);
    const int rounds = atoi(argv[2]);
    SphStateInfo info;
    char why[256];
    if (sph::state_parse(good.data(), good.size(), &info, why, sizeof(why)) != SPH_OK) { printf("the valid blob is refused: %s\n", why); return 1; }
    const unsigned long long extremes[6] = {0ull, 1ull, 0x7fffffffffffffffull, 0xffffffffffffffffull, 0xfffffffffffffff0ull, 0x100000000ull};
    int accepted = 0, refused = 0;
    for (int r = 0; r < rounds; ++r) {
        // a heap copy of exactly the mutated size: a read past its end is an AddressSanitizer report
        std::vector<unsigned char> m(good);
        switch (rnd() % 4) {
        case 0: for (int k = 1 + (int)(rnd() % 3); k > 0; --k) m[rnd() % m.size()] ^= (unsigned char)(1u << (rnd() % 8)); break;
        case 1: m.resize(rnd() % (m.size() + 1)); break;
        case 2: {   // a size field of the header or of the table set to an extreme
            const size_t fields[10] = {20, 24, 32, 40, 44, 256 + 8, 256 + 16, 256 + 40 + 8, 256 + 40 + 16, 256 + 0};
            const size_t at = fields[rnd() % 10];
            const unsigned long long v = extremes[rnd() % 6];
            memcpy(m.data() + at, &v, at == 20 || at == 40 || at == 44 || at == 256 ? 4 : 8);
            break;
        }
        default: {  // a word inside a payload's own record (counts of the core section) set to an extreme
            const size_t at = (size_t)info.offset[0] + 264 + 8 * (rnd() % 2);
            memcpy(m.data() + at, &extremes[rnd() % 6], 8);
            break;
        }
        }
        unsigned char* heap = (unsigned char*)malloc(m.size() ? m.size() : 1);
        memcpy(heap, m.data(), m.size());
        SphStateInfo out;
        const int rc = sph::state_parse(heap, m.size(), &out, why, sizeof(why));
        free(heap);
        if (rc == SPH_OK) {
            ++accepted;
            if (!sums_hold(m)) { printf("round %d: a blob with a broken checksum is accepted\n", r); return 1; }
            if (m != good) { printf("round %d: a blob that differs from the valid one is accepted\n", r); return 1; }
        } else {
            ++refused;
            if (rc != SPH_ERR_ARG || !why[0]) { printf("round %d: refusal %d without a message\n", r, rc); return 1; }
        }
    }
    printf("accepted %d refused %d\n", accepted, refused);
    return refused > 0 ? 0 : 1;
}
"""


@pytest.mark.parametrize("compiler", ["g++", "/opt/rocm/llvm/bin/clang++"])
def test_parser_under_sanitizers(pkg, scene, tmp_path, compiler):
    """state_parse (plain host C++, no HIP) fed a few thousand seeded mutations of a valid blob: bit flips, truncations, size fields at
    extremes.  No sanitizer report, and nothing accepted whose checksums do not hold."""
    cxx = shutil.which(compiler) or (compiler if os.path.exists(compiler) else None)
    if cxx is None:
        pytest.skip(f"{compiler} is not installed")
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    res = subprocess.run([cxx, *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if res.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip(f"{compiler} cannot link or start the sanitizer runtime: {res.stderr[-300:]}")
    src = tmp_path / "fuzz_state_parse.cpp"
    src.write_text(FUZZ_MAIN)
    exe = str(tmp_path / "fuzz_state_parse")
    res = subprocess.run([cxx, *flags, "-I", CSRC, str(src), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    blob = tmp_path / "good.blob"
    S.build_blob(pkg, *scene).tofile(str(blob))
    run = subprocess.run([exe, str(blob), "4000"], capture_output=True, text=True, timeout=120)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stdout + run.stderr
