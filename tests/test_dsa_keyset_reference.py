"""CPU: the groundwork of resident DSA key sets.  The window count, the digit extraction and the entry index of
bftkv_amd/csrc/dsa_verify.h compiled for the host (tests/c/dsa_keyset_host.cpp); a Python model of the key set that walks pow()
tables with those functions after dsav_prep_one and must reproduce the restatement of crypto/dsa.Verify (tests/dsa_verify_ref.py)
on every case of the seeded corpus, at window widths that divide the orders, that do not, and that straddle limbs; the new C-ABI
names; the scratch figures of the two new kernels."""
import os
import re
import subprocess

import numpy as np
import pytest

import dsa_keyset_host as KH
import dsa_verify_cases as K
import dsa_verify_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ["bftkv_gpu_dsa_keyset_create", "bftkv_gpu_dsa_keyset_destroy", "bftkv_gpu_dsa_keyset_info", "bftkv_gpu_dsa_verify_keyset",
             "bftkv_gpu_dsa_verify_keyset_dev", "bftkv_gpu_batcher_dsa_verify_keyset", "bftkv_gpu_selftest_dsa_keyset_table"]
NAMES = [g.name for g in K.groups() if g.pbytes <= 256]
WIDTHS = (4, 5, 8, 13)


@pytest.fixture(scope="module")
def dkh(tmp_path_factory):
    return KH.Host(KH.build(tmp_path_factory.mktemp("dks_host")))


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


def test_corpus_covers_what_the_chain_has_to_meet():
    """As tests/test_dsa_verify_reference.py asserts it: honest, mutated and constructed cases, a composite order, an order of odd
    width and p = 1 are all among the groups the model runs over."""
    kinds = {K.group(n).kind for n in NAMES}
    assert kinds == {"group", "composite", "odd_width", "p_one"}
    parts, have = set(), set()
    for n in NAMES:
        parts |= {cs.part for cs in K.corpus(n)}
        have |= {cs.label for cs in K.corpus(n)}
    assert parts == {"honest", "mutation", "constructed"}
    assert {"r + q", "g >= p", "g = p", "y = p", "y = p + 1", "u2 = 1", "digest = 0", "s = 3 and one byte more"} <= have
    assert {K.group(n).q.bit_length() for n in NAMES if K.group(n).kind == "group"} >= {160, 224, 256}
    assert any(K.group(n).p == 1 for n in NAMES)


def test_entry_index_is_the_documented_layout(dkh):
    """tab[base][window][d - 1], entries counted in rows of 76 limbs: the index function enumerates them in that order."""
    for w, windows, n_bases in ((4, 3, 3), (5, 2, 2), (8, 1, 2)):
        want = 0
        for base in range(n_bases):
            for i in range(windows):
                for d in range(1, 1 << w):
                    assert dkh.entry(base, i, d, windows, w) == want
                    want += 1
    # 64-bit: 8192 bases of 16 windows at w = 16
    assert dkh.entry(8191, 15, 65535, 16, 16) == 8192 * 16 * 65535 - 1


def test_window_counts(dkh):
    for qbits in (1, 8, 64, 160, 161, 224, 256):
        for w in range(4, 17):
            assert dkh.windows(qbits, w) == -(-qbits // w)
    # the top window is narrower where w does not divide the order's length
    assert [(dkh.windows(b, 5), dkh.windows(b, 13)) for b in (160, 224, 256)] == [(32, 13), (45, 18), (52, 20)]
    assert all(b % 5 and b % 13 for b in (224, 256)) and 160 % 13


def test_digits_recombine_to_the_exponent(dkh):
    q = K.group("dsa2048").q
    rng = np.random.default_rng(416)
    exps = [0, 1, q - 1, (1 << 256) - 1] + [1 << b for b in range(256)] + [int.from_bytes(rng.bytes(32), "big") for _ in range(64)]
    for e in exps:
        limbs = dkh.limbs10(e)
        assert KH.decode(limbs) == e
        for w in range(4, 17):
            n = dkh.windows(256, w)
            ds = dkh.digits(limbs, n, w)
            assert all(0 <= d < (1 << w) for d in ds)
            assert sum(d << (w * i) for i, d in enumerate(ds)) == e, (hex(e), w)
    # windows straddle two limbs at every width but 4, 7 and 14
    for w in range(4, 17):
        straddles = any((w * i) // 28 != (w * i + w - 1) // 28 for i in range(-(-256 // w)))
        assert straddles == (w not in (4, 7, 14)), w
    # a 160-bit exponent has only zero digits above window ceil(160 / w)
    e160 = K.group("dsa1024").q - 1
    assert e160.bit_length() == 160
    for e in (e160, (1 << 160) - 1):
        limbs = dkh.limbs10(e)
        for w in range(4, 17):
            n = dkh.windows(256, w)
            ds = dkh.digits(limbs, n, w)
            assert not any(ds[-(-160 // w):]) and ds[-(-160 // w) - 1] != 0, w


def test_pow_tables(dkh):
    """The model's table: entry (i, d) = b^(d 2^(w i)); in the device's form it is below p and decodes back through R."""
    G = K.group("p768_q64")
    for w in (4, 6):
        windows = dkh.windows(G.q.bit_length(), w)
        t = KH.table(G.y, G.p, w, windows)
        assert len(t) == windows and all(len(row) == (1 << w) - 1 for row in t)
        for i in (0, 1, windows - 1):
            for d in (1, 2, (1 << w) - 1):
                assert t[i][d - 1] == pow(G.y, d << (w * i), G.p)
        words = KH.table_words(G.y, G.p, w, windows)
        assert words.shape == (windows, (1 << w) - 1, KH.LIMBS) and int(words.max()) < (1 << 28)
        rinv = pow(KH.R, -1, G.p)
        assert KH.decode(words[0, 0]) < G.p and KH.decode(words[0, 0]) * rinv % G.p == G.y
        assert KH.decode(words[windows - 1, 2]) * rinv % G.p == pow(G.y, 3 << (w * (windows - 1)), G.p)


@pytest.mark.parametrize("name", NAMES)
def test_model_chain_over_the_corpus(dkh, name):
    """Every case of the corpus, at every width: the chain over the tables gives what crypto/dsa.Verify gives."""
    G = K.group(name)
    cases = K.corpus(name)
    gs, ks, idx = K.tables(cases)
    want = [V.verify(cs.p, cs.q, cs.g, cs.y, cs.digest, cs.r, cs.s) for cs in cases]
    assert len(gs) + len(ks) >= 8            # the mutated g and y make distinct bases
    for w in WIDTHS:
        m = KH.Model(dkh, gs, ks, w, G.qbytes)
        assert m.windows == -(-G.q.bit_length() // w)
        got = [m.verify(cs.digest, K.sig_bytes(G, cs.r, cs.s), ki) for cs, ki in zip(cases, idx)]
        bad = [(cs.label, wt, g) for cs, wt, g in zip(cases, want, got) if wt != g]
        assert not bad, (name, w, bad)
        if G.kind == "group":
            assert (1, V.OK) in got and (0, V.OK) in got
            top = m.windows - 1
            assert any(i == top for _, i, _ in m.touched) and any(i == 0 for _, i, _ in m.touched)
            if G.q.bit_length() % w:         # a narrower top window: its digits stay below 2^(bits(q) mod w)
                assert all(d < (1 << (G.q.bit_length() % w)) for _, i, d in m.touched if i == top)


def test_new_kernels_use_no_scratch(tmp_path):
    """k_dsav_comb_build<19, 4> and k_dsav_comb_exp<19, 4> for gfx950, from -Rpass-analysis=kernel-resource-usage: 0 bytes of scratch
    each (tests/c/dsa_keyset_kernels.hip instantiates these two and no other template of dsa_verify_kernels.hip)."""
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                        os.path.join(ROOT, "tests", "c", "dsa_keyset_kernels.hip"), "-o", str(tmp_path / "dks_kernels.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    found = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name and "k_dsav_comb_" in name:
            found[name] = int(m.group(1))
    print(found)
    assert len(found) == 2 and any("k_dsav_comb_build" in n for n in found) and any("k_dsav_comb_exp" in n for n in found), found
    assert not any(found.values()), found
