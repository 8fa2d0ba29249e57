"""-m gpu: ECDSA verification of raw signatures (crypto/ecdsa.Verify, Go 1.13) on the device over crypto/elliptic's four curves,
byte for byte (valid, status) against the restatement with its fence rules (tests/ecdsa_verify_ref.py)."""
import ctypes as C
import hashlib
import threading

import numpy as np
import pytest

import ec_ref as E
import ecdsa_verify_cases as K
import ecdsa_verify_ref as V

pytestmark = pytest.mark.gpu
E_INVALID, E_UNSUPPORTED = -1, -4
FAILED = 0xFF


def _want(c, cases):
    return [V.verify(c, cs.key, cs.digest, cs.sig) for cs in cases]


def _run(ctx, c, cases):
    """One device call per digest length (a call has one dlen), each case under its own key through key_idx."""
    got = [None] * len(cases)
    for dlen, idx in K.by_dlen(cases).items():
        keys = sorted({cases[i].key for i in idx})
        valid, st = ctx.ecdsa_verify([cases[i].digest for i in idx], [cases[i].sig for i in idx], keys, c,
                                     key_idx=[keys.index(cases[i].key) for i in idx])
        for j, i in enumerate(idx):
            got[i] = (int(valid[j]), int(st[j]))
    return got


@pytest.mark.parametrize("name", E.NAMES)
def test_corpus(gpu_ctx, name):
    c = E.CURVES[name]
    cases = K.corpus(name)
    want, got = _want(c, cases), _run(gpu_ctx, c, cases)
    for cs, w, g in zip(cases, want, got):
        print(name, cs.label, "want", w, "got", g)
    bad = [(cs.label, w, g) for cs, w, g in zip(cases, want, got) if w != g]
    assert not bad, (name, bad)
    assert sum(w == (1, V.OK) for w in want) >= 14 and sum(w[1] == V.FENCED for w in want) >= 8
    assert sum(cs.group == "special_x" and w == (1, V.OK) for cs, w in zip(cases, want)) >= 2           # R at the special x
    assert sum(cs.group == "special_x" and w == (0, V.OK) for cs, w in zip(cases, want)) >= 3           # ... and with r + 1
    # a lone call, and NULL key_idx meaning key 0
    for i in (0, len(cases) - 1):
        cs = cases[i]
        valid, st = gpu_ctx.ecdsa_verify([cs.digest], [cs.sig], [cs.key], c)
        assert (int(valid[0]), int(st[0])) == want[i], (name, cs.label)


def _signed_batch(ctx, c, rng, n_ops, n_keys, dlen):
    """n_ops honest signatures under n_keys keys (k G and d G from the device's ScalarBaseMult), every 7th one mutated."""
    n, f = c["n"], E.byte_len(c)
    ds = [K.rnd(rng, c) or 1 for _ in range(n_keys)]
    ks = [K.rnd(rng, c) or 1 for _ in range(n_ops)]
    pts, st = ctx.ec_scalar_base_mult(ds + ks, c)
    assert not st.any()
    keys = pts[:n_keys]
    key_idx = [int(v) for v in rng.integers(n_keys, size=n_ops)]
    digests, sigs, expect = [], [], []
    for i in range(n_ops):
        dg = rng.bytes(dlen)
        r = int.from_bytes(pts[n_keys + i][1:1 + f], "big") % n
        s = pow(ks[i], -1, n) * (V.hash_to_int(c, dg) + r * ds[key_idx[i]]) % n
        sg = K.sig_bytes(c, r, s)
        ok = 1
        if i % 7 == 3:
            ok = 0
            which = (i // 7) % 4
            if which == 0:
                sg = K.flip(sg, int(rng.integers(8 * f)))
            elif which == 1:
                sg = K.flip(sg, 8 * f + int(rng.integers(8 * f)))
            elif which == 2:
                dg = K.flip(dg, int(rng.integers(8 * min(dlen, f) - 8)))
            elif n_keys > 1:
                key_idx[i] = (key_idx[i] + 1) % n_keys
            else:
                sg = sg[f:] + sg[:f]
        digests.append(dg)
        sigs.append(sg)
        expect.append(ok)
    return digests, sigs, keys, key_idx, np.array(expect, dtype=np.uint8)


@pytest.mark.parametrize("n_keys", [1, 1000])
@pytest.mark.parametrize("name", E.NAMES)
def test_ten_thousand(gpu_ctx, name, n_keys):
    c = E.CURVES[name]
    rng = np.random.default_rng(31 * c["bit_size"] + n_keys)
    dlen = {"P-224": 28, "P-256": 32, "P-384": 48, "P-521": 64}[name]
    digests, sigs, keys, key_idx, expect = _signed_batch(gpu_ctx, c, rng, 10000, n_keys, dlen)
    valid, st = gpu_ctx.ecdsa_verify(digests, sigs, keys, c, key_idx=None if n_keys == 1 else key_idx)
    assert not st.any(), (name, np.flatnonzero(st)[:8])                 # nothing fenced, nothing failed
    assert (valid == expect).all(), (name, np.flatnonzero(valid != expect)[:8])
    assert expect.sum() == 10000 - len(range(3, 10000, 7))
    for i in [int(v) for v in rng.choice(10000, 12, replace=False)] + [3, 10, 17, 24]:
        assert (int(valid[i]), int(st[i])) == V.verify(c, keys[key_idx[i] if n_keys > 1 else 0], digests[i], sigs[i]), (name, i)


def test_key_index_is_clamped(gpu_ctx):
    c = E.CURVES["P-256"]
    rng = np.random.default_rng(5)
    digests, sigs, keys, key_idx, expect = _signed_batch(gpu_ctx, c, rng, 6, 2, 32)
    want = [V.verify(c, keys[min(i, 1)], digests[j], sigs[j]) for j, i in enumerate([0, 1, 2, 7, 0xFFFFFFFF, 1])]
    valid, st = gpu_ctx.ecdsa_verify(digests, sigs, keys, c, key_idx=[0, 1, 2, 7, 0xFFFFFFFF, 1])
    assert [(int(v), int(s)) for v, s in zip(valid, st)] == want


def test_device_form_against_host_form(gpu_ctx):
    import torch
    from bftkv_amd._native import _curve_bytes
    lib, h = gpu_ctx.lib, gpu_ctx.h
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")    # noqa: E731
    for name in E.NAMES:
        c = E.CURVES[name]
        f = E.byte_len(c)
        cases = [cs for cs in K.corpus(name) if len(cs.digest) == f]
        keys = sorted({cs.key for cs in cases})
        idx = [keys.index(cs.key) for cs in cases]
        n_ops = len(cases)
        valid, st = gpu_ctx.ecdsa_verify([cs.digest for cs in cases], [cs.sig for cs in cases], keys, c, key_idx=idx)
        assert [(int(v), int(s)) for v, s in zip(valid, st)] == _want(c, cases)
        assert st.any() and valid.any()
        cb, bits, _ = _curve_bytes(c)
        kb = np.frombuffer(b"".join(keys), dtype=np.uint8).copy()
        d_dg = up(np.frombuffer(b"".join(cs.digest for cs in cases), dtype=np.uint8).copy())
        d_sg = up(np.frombuffer(b"".join(cs.sig for cs in cases), dtype=np.uint8).copy())
        d_ki = up(np.array(idx, dtype=np.uint32).view(np.int32))
        d_valid = torch.full((n_ops + 8,), 0x55, dtype=torch.uint8, device="cuda:0")
        d_st = torch.full((n_ops + 8,), 0x55, dtype=torch.uint8, device="cuda:0")
        gpu_ctx._check(lib.bftkv_gpu_ecdsa_verify_dev(h, n_ops, d_dg.data_ptr(), f, d_sg.data_ptr(), d_ki.data_ptr(), len(keys),
                                                      kb.ctypes.data_as(C.c_void_p), cb.ctypes.data_as(C.c_void_p), bits, d_valid.data_ptr(),
                                                      d_st.data_ptr()), "ecdsa_verify_dev")
        gpu_ctx.sync()
        assert (d_valid.cpu().numpy()[:n_ops] == valid).all() and (d_st.cpu().numpy()[:n_ops] == st).all(), name
        assert (d_valid.cpu().numpy()[n_ops:] == 0x55).all() and (d_st.cpu().numpy()[n_ops:] == 0x55).all()      # nothing past n_ops


def test_batcher_mixed_curves(gpu_ctx):
    from bftkv_amd import Batcher
    jobs = []
    for name in E.NAMES:
        c = E.CURVES[name]
        jobs += [(c, cs) for cs in K.corpus(name)]
    rng = np.random.default_rng(77)
    jobs = [jobs[int(i)] for i in rng.permutation(len(jobs))]
    want = [V.verify(c, cs.key, cs.digest, cs.sig) for c, cs in jobs]
    assert {w for w in want} == {(1, V.OK), (0, V.OK), (0, V.FENCED)}
    b = Batcher(gpu_ctx, max_items=64, n_lanes=2)
    got = [None] * len(jobs)

    def run(lo):
        for i in range(lo, len(jobs), 32):
            c, cs = jobs[i]
            got[i] = b.ecdsa_verify(cs.digest, cs.sig, cs.key, c)

    th = [threading.Thread(target=run, args=(i,)) for i in range(32)]
    for t_ in th:
        t_.start()
    for t_ in th:
        t_.join()
    b.close()
    for i, (w, g) in enumerate(zip(want, got)):
        assert g == (0, w[1], w[0]), (i, jobs[i][1].label, w, g)


@pytest.mark.parametrize("name", E.NAMES)
def test_real_threshold_signature_verifies_on_the_device(gpu_ctx, name):
    """The construction of test_gpu_threshold_ecdsa.py::test_real_threshold_signature (the Sign math of dsa_core.go:120-161): r from
    the device's CalculateR, s from the device's lagrange_combine, and now the verdict from the device as well: VALID; INVALID
    after one partial share is corrupted."""
    c = E.CURVES[name]
    n, f = c["n"], E.byte_len(c)
    rng = np.random.default_rng(1000 + c["bit_size"])
    t, xs = 3, list(range(1, 9))

    def share(secret):
        coef = [secret] + [K.rnd(rng, c) for _ in range(t)]
        return [sum(a * x ** i for i, a in enumerate(coef)) % n for x in xs]

    d, k, a = (K.rnd(rng, c) for _ in range(3))
    di, ki, ai = share(d), share(k), share(a)
    vi = [x * y % n for x, y in zip(ki, ai)]
    ri, st = gpu_ctx.ec_scalar_base_mult(ai, c)
    assert not st.any()
    (r,), st = gpu_ctx.ecdsa_calculate_r([xs], [ri], [vi], c)
    assert not st.any()
    hname = {"P-224": "sha224", "P-256": "sha256", "P-384": "sha384", "P-521": "sha512"}[name]
    digest = hashlib.new(hname, b"bftkv threshold ecdsa").digest()
    e = V.hash_to_int(c, digest)
    si = [kk * (e + r * dd) % n for kk, dd in zip(ki, di)]
    bad = list(si)
    bad[2] = (bad[2] + 1) % n
    (s, s_bad), st = gpu_ctx.lagrange_combine([xs, xs], [si, bad], [n], [0, 0], nbytes=f)
    assert not st.any() and s != s_bad
    (q,), st = gpu_ctx.ec_scalar_base_mult([d], c)
    assert not st.any()
    valid, st = gpu_ctx.ecdsa_verify([digest, digest], [K.sig_bytes(c, r, s), K.sig_bytes(c, r, s_bad)], [q], c)
    assert [int(v) for v in valid] == [1, 0] and not st.any()
    assert V.verify(c, q, digest, K.sig_bytes(c, r, s)) == (1, V.OK) and V.verify(c, q, digest, K.sig_bytes(c, r, s_bad)) == (0, V.OK)


def test_errors(gpu_ctx):
    from bftkv_amd._native import NativeError, _curve_bytes
    c = E.CURVES["P-256"]
    cs = K.corpus("P-256")[0]
    other = dict(c, b=c["b"] ^ 1)
    with pytest.raises(NativeError, match=r"\(-4\)"):
        gpu_ctx.ecdsa_verify([cs.digest], [cs.sig], [cs.key], other)
    lib, h = gpu_ctx.lib, gpu_ctx.h
    cb, bits, _ = _curve_bytes(c)
    cb2, bits2, _ = _curve_bytes(other)
    buf = np.zeros(4096, dtype=np.uint8)
    P = lambda a: a.ctypes.data_as(C.c_void_p)        # noqa: E731
    valid, st = np.full(8, 0xAA, dtype=np.uint8), np.full(8, 0xAA, dtype=np.uint8)
    call = lambda *a: lib.bftkv_gpu_ecdsa_verify(*a)     # noqa: E731
    assert call(None, 1, P(buf), 32, P(buf), None, 1, P(buf), P(cb), bits, P(valid), P(st)) == E_INVALID
    assert call(h, 1, None, 32, P(buf), None, 1, P(buf), P(cb), bits, P(valid), P(st)) == E_INVALID
    assert call(h, 1, P(buf), 32, None, None, 1, P(buf), P(cb), bits, P(valid), P(st)) == E_INVALID
    assert call(h, 1, P(buf), 32, P(buf), None, 1, None, P(cb), bits, P(valid), P(st)) == E_INVALID
    assert call(h, 1, P(buf), 32, P(buf), None, 1, P(buf), None, bits, P(valid), P(st)) == E_INVALID
    assert call(h, 1, P(buf), 32, P(buf), None, 1, P(buf), P(cb), bits, None, P(st)) == E_INVALID
    assert call(h, 1, P(buf), 32, P(buf), None, 1, P(buf), P(cb), bits, P(valid), None) == E_INVALID
    assert call(h, 1, P(buf), 32, P(buf), None, 0, P(buf), P(cb), bits, P(valid), P(st)) == E_INVALID          # n_keys = 0
    assert call(h, 1, P(buf), 0, P(buf), None, 1, P(buf), P(cb), bits, P(valid), P(st)) == E_INVALID           # dlen = 0
    assert call(h, 1, P(buf), 67, P(buf), None, 1, P(buf), P(cb), bits, P(valid), P(st)) == E_INVALID          # dlen > 66
    assert call(h, 1, P(buf), 32, P(buf), None, 1, P(buf), P(cb), 0, P(valid), P(st)) == E_INVALID
    assert call(h, 1, P(buf), 32, P(buf), None, 1, P(buf), P(cb2), bits2, P(valid), P(st)) == E_UNSUPPORTED
    assert call(h, 1, P(buf), 32, P(buf), None, 1, P(buf), P(cb), 255, P(valid), P(st)) == E_UNSUPPORTED
    assert (valid == 0xAA).all() and (st == 0xAA).all()                      # refused calls touch nothing
    assert call(h, 0, None, 32, None, None, 1, P(buf), P(cb), bits, None, None) == 0
    # an all-zero key is no point: fenced, and dlen = 66 on P-256 is the leftmost 32 bytes
    assert call(h, 1, P(buf), 66, P(buf), None, 1, P(buf), P(cb), bits, P(valid), P(st)) == 0
    assert (int(valid[0]), int(st[0])) == (0, V.FENCED)
    v1, s1 = np.full(1, 0xAA, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
    assert lib.bftkv_gpu_batcher_ecdsa_verify(None, P(buf), 32, P(buf), P(buf), P(cb), bits, P(v1), P(s1)) == E_INVALID
    assert (int(v1[0]), int(s1[0])) == (0, FAILED)
    from bftkv_amd import Batcher
    b = Batcher(gpu_ctx, max_items=8, n_lanes=1)
    v1[0], s1[0] = 0xAA, 0
    assert lib.bftkv_gpu_batcher_ecdsa_verify(b.h, P(buf), 32, P(buf), P(buf), P(cb2), bits2, P(v1), P(s1)) == E_UNSUPPORTED
    assert (int(v1[0]), int(s1[0])) == (0, FAILED)
    assert lib.bftkv_gpu_batcher_ecdsa_verify(b.h, P(buf), 0, P(buf), P(buf), P(cb), bits, P(v1), P(s1)) == E_INVALID
    key = np.frombuffer(cs.key, dtype=np.uint8).copy()
    dg, sg = np.frombuffer(cs.digest, dtype=np.uint8).copy(), np.frombuffer(cs.sig, dtype=np.uint8).copy()
    assert lib.bftkv_gpu_batcher_ecdsa_verify(b.h, P(dg), len(cs.digest), P(sg), P(key), P(cb), bits, P(v1), P(s1)) == 0
    assert (int(v1[0]), int(s1[0])) == (1, V.OK)
    b.close()
