"""CPU: the groundwork of resident ECDSA key sets.  fb_table_build of bftkv_amd/csrc/ec_field.h over an arbitrary base point
(compiled for the host: tests/c/ecdsa_keyset_host.cpp) against tests/ec_ref.py, fb_mul over such tables, the verification chain
in the kernels' order with the key's table against tests/ecdsa_verify_ref.py over the whole corpus, the new C-ABI names, and the
register / scratch figures of the new kernels from the compiler's remarks."""
import os
import re
import subprocess

import numpy as np
import pytest

import ec_ref as E
import ecdsa_keyset_host as KH
import ecdsa_verify_cases as K
import ecdsa_verify_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ["bftkv_gpu_ecdsa_keyset_create", "bftkv_gpu_ecdsa_keyset_destroy", "bftkv_gpu_ecdsa_keyset_info", "bftkv_gpu_ecdsa_verify_keyset",
             "bftkv_gpu_ecdsa_verify_keyset_dev", "bftkv_gpu_batcher_ecdsa_verify_keyset", "bftkv_gpu_selftest_ecdsa_keyset_table"]


@pytest.fixture(scope="module")
def ekh(tmp_path_factory):
    return KH.build(tmp_path_factory.mktemp("eks_host"))


def smul(c, pt, k: int):
    return E.scalar_mult(c, pt[0], pt[1], E.int_bytes(k))


def check_table(h, words, w, base):
    """Every entry j of every window i is ec_ref.scalar_mult(base, j 2^(w i)).  By induction over short scalars (a full-width
    scalar per entry would be two thousand ladders per P-521 table): entry (0, 1) is the base, entry (i, 1) is 2^w times entry
    (i - 1, 1), entry (i, j) is j times entry (i, 1) -- each through ec_ref.scalar_mult; the corners and a seeded sample are
    checked against the full-width scalar directly as well.  Slot 0 of every run is zero."""
    c = h.c
    n, L = c["n"], h.L
    nwin = KH.windows(c, w)
    assert len(words) == KH.table_words(c, w)
    assert not words.reshape(nwin * 2 * L, 1 << w)[:, 0].any()
    first = base
    for i in range(nwin):
        if i:
            first = smul(c, first, 1 << w)
        for j in range(1, 1 << w):
            assert h.entry(words, w, i, j) == (first if j == 1 else smul(c, first, j)), (w, i, j)
    rng = np.random.default_rng(w)
    picks = [(0, 1), (0, (1 << w) - 1), (nwin - 1, 1), (nwin - 1, (1 << w) - 1)]
    picks += [(int(rng.integers(nwin)), int(rng.integers(1, 1 << w))) for _ in range(4)]
    for i, j in picks:
        assert h.entry(words, w, i, j) == smul(c, base, (j << (w * i)) % n), (w, i, j)


@pytest.mark.parametrize("name", E.NAMES)
def test_g_table_unchanged(ekh, name):
    """The generalised fb_table_build with base G: the words of the overload that takes no base, and j 2^(w i) G by ec_ref."""
    c = E.CURVES[name]
    h = KH.Host(ekh, c)
    g = (c["gx"], c["gy"])
    for w in (4, 5):
        words = h.table(w, None)
        assert (h.table(w, g) == words).all(), (name, w)
        check_table(h, words, w, g)


def _bases(c):
    rng = np.random.default_rng(40 + c["bit_size"])
    return [E.scalar_base_mult(c, K.rnd(rng, c) or 1) for _ in range(2)]


@pytest.mark.parametrize("name", E.NAMES)
def test_table_of_an_arbitrary_base(ekh, name):
    c = E.CURVES[name]
    h = KH.Host(ekh, c)
    for q in _bases(c):
        for w in (2, 4, 5):
            check_table(h, h.table(w, q), w, q)


@pytest.mark.parametrize("name", E.NAMES)
def test_fb_mul_over_a_key_table(ekh, name):
    c = E.CURVES[name]
    h = KH.Host(ekh, c)
    rng = np.random.default_rng(41 + c["bit_size"])
    for q in _bases(c):
        for w in (2, 4, 5):
            for k in KH.chosen_scalars(c, w, rng):
                assert h.mul(w, q, k) == smul(c, q, k), (name, w, hex(k))
            assert h.mul(w, q, 0) == (0, 0)


@pytest.mark.parametrize("name", E.NAMES)
def test_chain_in_the_kernels_order_over_the_corpus(ekh, name):
    """hash_to_int, fn_mul, fb_mul on G, the refusal flag or fb_mul on the key's table, pt_add and x_matches_r, strung together
    as k_ecv_prep / k_ecv_base / k_ecv_key_tab string them: ecdsa_verify_ref.verify's answer on every case."""
    c = E.CURVES[name]
    h = KH.Host(ekh, c)
    want = [V.verify(c, cs.key, cs.digest, cs.sig) for cs in K.corpus(name)]
    for cs, wt in zip(K.corpus(name), want):
        assert h.verify(4, cs.key, cs.sig, cs.digest) == wt, (name, cs.label)
    assert sum(wt == (1, V.OK) for wt in want) >= 14 and sum(wt[1] == V.FENCED for wt in want) >= 8
    for cs, wt in list(zip(K.corpus(name), want))[::5]:
        assert h.verify(5, cs.key, cs.sig, cs.digest) == wt, (name, cs.label, "w = 5")


def test_keyset_names_declared_and_exported():
    import __graft_entry__ as ge
    from bftkv_amd import _native
    hdr = open(os.path.join(ROOT, "include", "bftkv_gpu.h")).read()
    declared = set(re.findall(r"\b(bftkv_gpu_[a-z_0-9]+)\s*\(", hdr))
    for name in NEW_NAMES:
        assert name in declared and name in _native.EXPORTS, name
    ge.build()
    lib = _native.load_library()
    for name in NEW_NAMES:
        assert hasattr(lib, name), name


def test_new_kernels_use_no_scratch(tmp_path):
    """k_ec_keytab_build and k_ecv_key_tab for gfx950 on all four curves, from -Rpass-analysis=kernel-resource-usage: 0 bytes of
    scratch each (tests/c/ecdsa_keyset_kernels.hip instantiates exactly these eight)."""
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                        os.path.join(ROOT, "tests", "c", "ecdsa_keyset_kernels.hip"), "-o", str(tmp_path / "eks_kernels.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    found = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name and ("k_ec_keytab_build" in name or "k_ecv_key_tab" in name):
            found[name] = int(m.group(1))
    print(found)
    assert len(found) == 8, found
    assert not any(found.values()), found
