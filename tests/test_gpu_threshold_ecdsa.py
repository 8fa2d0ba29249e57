"""-m gpu: threshold ECDSA (crypto/threshold/ecdsa/ecdsa.go) on the device -- CalculateR and CalculatePartialR over
crypto/elliptic's four curves, byte-exact against the restatement of Go's generic curve code (tests/ec_ref.py)."""
import ctypes as C
import hashlib
import threading

import numpy as np
import pytest

import ec_ref as E
from oracle.threshold import lagrange

pytestmark = pytest.mark.gpu
E_INVALID, E_UNSUPPORTED = -1, -4


def _rnd(rng, c, m=None):
    return int.from_bytes(rng.bytes(E.byte_len(c) + 8), "big") % (m or c["n"])


def _xs(rng, k):
    if k <= 8:
        return list(range(1, k + 1))
    return [int(v) for v in rng.permutation(255 if k > 22 else 64)[:k] + 1]


def _base_points(ctx, c, scalars):
    pts, st = ctx.ec_scalar_base_mult(scalars, c)
    assert not st.any()
    return pts


def _identity_ops(ctx, c, rng, n_ops, k, random_xs=True):
    """TestMul's shape (ecdsa_test.go): R_i = f(x_i) G, V_i = f(x_i) for a polynomial f: CalculateR = Gx mod N."""
    n = c["n"]
    xs, fx = [], []
    for _ in range(n_ops):
        x = _xs(rng, k) if random_xs else list(range(1, k + 1))
        coef = [_rnd(rng, c) for _ in range(min(k, 4))]
        xs.append(x)
        fx.append([sum(a * pow(xi, i, n) for i, a in enumerate(coef)) % n for xi in x])
    pts = _base_points(ctx, c, [v for row in fx for v in row])
    return xs, [pts[i * k:(i + 1) * k] for i in range(n_ops)], fx


def _random_ops(ctx, c, rng, n_ops, k):
    xs = [_xs(rng, k) for _ in range(n_ops)]
    pts = _base_points(ctx, c, [_rnd(rng, c) for _ in range(n_ops * k)])
    vi = [[_rnd(rng, c) for _ in range(k)] for _ in range(n_ops)]
    return xs, [pts[i * k:(i + 1) * k] for i in range(n_ops)], vi


@pytest.mark.parametrize("name", E.NAMES)
def test_calculate_r_every_curve_and_width(gpu_ctx, name):
    c = E.CURVES[name]
    rng = np.random.default_rng(100 + c["bit_size"])
    gx = c["gx"] % c["n"]
    for k in (1, 2, 8, 22, 64):
        xi, ri, vi = _identity_ops(gpu_ctx, c, rng, 34, k)
        xr, rr, vr = _random_ops(gpu_ctx, c, rng, 3, k)
        xs, rs, vs = xr + xi, rr + ri, vr + vi                      # 37 operations
        got, st = gpu_ctx.ecdsa_calculate_r(xs, rs, vs, c)
        assert not st.any(), (name, k, st)
        assert got[3:] == [gx] * 34, (name, k)
        for i in range(3 if k <= 22 else 1):
            assert (int(st[i]), got[i]) == E.calculate_r(c, xs[i], rs[i], vs[i]), (name, k, i)
        one, st1 = gpu_ctx.ecdsa_calculate_r(xs[:1], rs[:1], vs[:1], c)   # a lone call
        assert one == got[:1] and not st1.any()


@pytest.mark.parametrize("name", E.NAMES)
def test_calculate_r_ten_thousand(gpu_ctx, name):
    c = E.CURVES[name]
    rng = np.random.default_rng(7 + c["bit_size"])
    xs, ri, vi = _identity_ops(gpu_ctx, c, rng, 10000, 8, random_xs=False)
    sample = sorted(int(v) for v in rng.choice(10000, 200, replace=False))
    xr, rr, vr = _random_ops(gpu_ctx, c, rng, len(sample), 8)
    for j, i in enumerate(sample):
        xs[i], ri[i], vi[i] = xr[j], rr[j], vr[j]
    got, st = gpu_ctx.ecdsa_calculate_r(xs, ri, vi, c)
    assert not st.any()
    sset = set(sample)
    assert all(got[i] == c["gx"] % c["n"] for i in range(10000) if i not in sset)
    for i in sample:
        assert (int(st[i]), got[i]) == E.calculate_r(c, xs[i], ri[i], vi[i]), i


def _edge_ops(gpu_ctx, c, rng):
    n, p, f = c["n"], c["p"], E.byte_len(c)
    ops = []
    xs = [1, 2, 3, 4]
    base = lambda k: _random_ops(gpu_ctx, c, rng, 1, k)           # noqa: E731
    _, (ri,), (vi,) = base(4)
    ops.append(([0, 2, 3, 4], ri, vi))                            # a share index 0: l_j = 0 for the others
    ops.append(([1, 2, 2, 4], ri, vi))                            # duplicate x
    ls = [lagrange(x, xs, n) for x in xs]
    a = _rnd(rng, c)
    r0, r1 = _base_points(gpu_ctx, c, [a, a * ls[0] * pow(ls[1], -1, n) % n])
    ops.append((xs, [r0, r1] + ri[2:], vi))                       # T_0 = T_1: Add's doubling case
    r1n = _base_points(gpu_ctx, c, [(-a * ls[0] * pow(ls[1], -1, n)) % n])[0]
    ops.append((xs, [r0, r1n] + ri[2:], vi))                      # T_1 = -T_0 mid-fold
    l2 = [lagrange(x, [1, 2], n) for x in (1, 2)]
    r1f = _base_points(gpu_ctx, c, [(-a * l2[0] * pow(l2[1], -1, n)) % n])[0]
    ops.append(([1, 2], [r0, r1f], vi[:2]))                       # ... as the final fold: r = 0
    v0 = list(vi)
    v0[3] = (-sum(v * l for v, l in zip(vi[:3], ls[:3])) * pow(ls[3], -1, n)) % n
    ops.append((xs, ri, v0))                                      # v = 0
    x0, y0 = int.from_bytes(ri[1][1:1 + f], "big"), int.from_bytes(ri[1][1 + f:], "big")
    for bad in (b"\x02" + ri[1][1:], E.marshal(c, x0, (y0 + 1) % p), E.marshal(c, p, y0), E.marshal(c, x0, p), E.marshal(c, 0, 0)):
        ops.append((xs, [ri[0], bad] + ri[2:], vi))               # Unmarshal refuses
    return ops


@pytest.mark.parametrize("name", E.NAMES)
def test_calculate_r_edges(gpu_ctx, name):
    c = E.CURVES[name]
    rng = np.random.default_rng(55 + c["bit_size"])
    ops = _edge_ops(gpu_ctx, c, rng)
    want = [E.calculate_r(c, *o) for o in ops]
    assert [w[0] for w in want] == [E.FENCED, E.OK, E.FENCED, E.FENCED, E.OK, E.NO_INVERSE] + [E.FENCED] * 5
    assert want[4] == (E.OK, 0)
    for k in (2, 4):
        sel = [i for i, o in enumerate(ops) if len(o[0]) == k]
        got, st = gpu_ctx.ecdsa_calculate_r([ops[i][0] for i in sel], [ops[i][1] for i in sel], [ops[i][2] for i in sel], c)
        assert [(int(s), r) for s, r in zip(st, got)] == [want[i] for i in sel], name


def _needs_big(x):
    """k_lagrange_inv's rule: some numerator or denominator product leaves 31 bits."""
    for xj in x:
        a = b = 1
        for xi in x:
            if xi == xj:
                continue
            a, b = a * xi, b * (xi - xj)
            if abs(a) >= 1 << 31 or abs(b) >= 1 << 31:
                return True
    return False


def test_big_path_bound_and_device_form(gpu_ctx):
    import torch
    from bftkv_amd._native import _curve_bytes, _ints_to_be
    c = E.CURVES["P-256"]
    rng = np.random.default_rng(64)
    # k = 64 with indices up to 255: every operation through the big Lagrange path
    xs, ri, vi = _random_ops(gpu_ctx, c, rng, 2, 64)
    xs_i, ri_i, vi_i = _identity_ops(gpu_ctx, c, rng, 30, 64)
    got, st = gpu_ctx.ecdsa_calculate_r(xs + xs_i, ri + ri_i, vi + vi_i, c)
    assert not st.any() and got[2:] == [c["gx"] % c["n"]] * 30
    assert all((int(st[i]), got[i]) == E.calculate_r(c, xs[i], ri[i], vi[i]) for i in range(2))
    # the device form at k = 8, indices up to 60, with and without a promised bound on the x's
    n_ops, k, f = 40, 8, 32
    xs = [[int(v) for v in rng.permutation(60)[:k] + 1] for _ in range(n_ops)]
    ri = [r for r in _random_ops(gpu_ctx, c, rng, n_ops, k)[1]]
    vi = [[_rnd(rng, c) for _ in range(k)] for _ in range(n_ops)]
    host, st = gpu_ctx.ecdsa_calculate_r(xs, ri, vi, c)
    assert not st.any() and (int(st[0]), host[0]) == E.calculate_r(c, xs[0], ri[0], vi[0])
    big = np.array([_needs_big(x) for x in xs])
    assert big.sum() > n_ops // 2
    lib, h = gpu_ctx.lib, gpu_ctx.h
    cb, bits, _ = _curve_bytes(c)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")    # noqa: E731
    d_x = up(np.array(xs, dtype=np.int32))
    d_r = up(np.frombuffer(b"".join(bytes(p) for row in ri for p in row), dtype=np.uint8).copy())
    d_v = up(_ints_to_be([v for row in vi for v in row], f))
    for bound, ok in ((0, True), (60, True), (10, False), (0, True)):
        gpu_ctx._check(lib.bftkv_gpu_set_lagrange_x_bound(h, bound), "set_lagrange_x_bound")
        o = torch.zeros((n_ops, f), dtype=torch.uint8, device="cuda:0")
        s = torch.zeros(n_ops + 8, dtype=torch.uint8, device="cuda:0")
        gpu_ctx._check(lib.bftkv_gpu_ecdsa_calculate_r_dev(h, n_ops, k, d_x.data_ptr(), d_r.data_ptr(), d_v.data_ptr(),
                                                           cb.ctypes.data_as(C.c_void_p), bits, o.data_ptr(), s.data_ptr()), "ecdsa_dev")
        gpu_ctx.sync()
        got = [int.from_bytes(r.tobytes(), "big") for r in o.cpu().numpy()]
        stn = s.cpu().numpy()[:n_ops]
        if ok:
            assert not stn.any() and got == host, bound
        else:                                                        # a broken promise costs a fence, never a wrong number
            assert (stn[big] == E.FENCED).all() and not stn[~big].any()
            assert [g for g, b_ in zip(got, big) if b_] == [0] * int(big.sum())
            assert [g for g, b_ in zip(got, big) if not b_] == [w for w, b_ in zip(host, big) if not b_]
    gpu_ctx._check(lib.bftkv_gpu_set_lagrange_x_bound(h, 0), "set_lagrange_x_bound")


@pytest.mark.parametrize("name", E.NAMES)
def test_scalar_base_mult(gpu_ctx, name):
    c = E.CURVES[name]
    n = c["n"]
    rng = np.random.default_rng(9)
    scalars = [0, 1, 2, n - 1, n] + [_rnd(rng, c) for _ in range(20)]
    out, st = gpu_ctx.ec_scalar_base_mult(scalars, c)
    f = E.byte_len(c)
    for s, o, t in zip(scalars, out, st):
        if s >= n:
            assert t == E.FENCED and o == bytes(1 + 2 * f)
        else:
            assert t == E.OK and o == E.calculate_partial_r(c, s), s
    assert out[0] == b"\x04" + bytes(2 * f)


def _openssl_verify(name, q, digest, r, s):
    try:
        lib = C.CDLL("libcrypto.so.3")
    except OSError:
        return None
    vp = C.c_void_p
    nid = {"P-224": 713, "P-256": 415, "P-384": 715, "P-521": 716}[name]
    lib.EC_KEY_new_by_curve_name.restype, lib.EC_KEY_new_by_curve_name.argtypes = vp, [C.c_int]
    lib.EC_KEY_set_public_key_affine_coordinates.argtypes = [vp, vp, vp]
    lib.BN_bin2bn.restype, lib.BN_bin2bn.argtypes = vp, [C.c_char_p, C.c_int, vp]
    lib.ECDSA_SIG_new.restype = vp
    lib.ECDSA_SIG_set0.argtypes = [vp, vp, vp]
    lib.ECDSA_do_verify.argtypes = [C.c_char_p, C.c_int, vp, vp]
    bn = lambda v: lib.BN_bin2bn(E.int_bytes(v) or b"\x00", len(E.int_bytes(v) or b"\x00"), None)   # noqa: E731
    key = lib.EC_KEY_new_by_curve_name(nid)
    assert lib.EC_KEY_set_public_key_affine_coordinates(key, bn(q[0]), bn(q[1])) == 1
    sig = lib.ECDSA_SIG_new()
    assert lib.ECDSA_SIG_set0(sig, bn(r), bn(s)) == 1
    return lib.ECDSA_do_verify(digest, len(digest), sig, key) == 1


@pytest.mark.parametrize("name", E.NAMES)
def test_real_threshold_signature(gpu_ctx, name):
    """The Sign math of dsa_core.go:120-161 on ECDSA: shares of d, k and a (degree t), Vi = k_i a_i (degree 2t), partial Rs from
    the device's ScalarBaseMult, r from the device's CalculateR (x of (a k)^-1 a G = k^-1 G), s = sum l_i k_i (e + r d_i) from the
    existing lagrange_combine mod N: (r, s) verifies under d G."""
    c = E.CURVES[name]
    n, f = c["n"], E.byte_len(c)
    rng = np.random.default_rng(1000 + c["bit_size"])
    t, xs = 3, list(range(1, 9))
    def share(secret):
        coef = [secret] + [_rnd(rng, c) for _ in range(t)]
        return [sum(a * x ** i for i, a in enumerate(coef)) % n for x in xs]
    d, k, a = (_rnd(rng, c) for _ in range(3))
    di, ki, ai = share(d), share(k), share(a)
    vi = [x * y % n for x, y in zip(ki, ai)]
    ri = _base_points(gpu_ctx, c, ai)
    (r,), st = gpu_ctx.ecdsa_calculate_r([xs], [ri], [vi], c)
    assert not st.any() and r == E.scalar_base_mult(c, pow(k, -1, n))[0] % n
    assert (E.OK, r) == E.calculate_r(c, xs, ri, vi)
    hname = {"P-224": "sha224", "P-256": "sha256", "P-384": "sha384", "P-521": "sha512"}[name]
    digest = hashlib.new(hname, b"bftkv threshold ecdsa").digest()
    e = int.from_bytes(digest, "big")
    si = [kk * (e + r * dd) % n for kk, dd in zip(ki, di)]
    (s,), st = gpu_ctx.lagrange_combine([xs], [si], [n], [0], nbytes=f)
    assert not st.any()
    q = E.scalar_base_mult(c, d)
    assert E.ecdsa_verify(c, q, e, r, s)
    assert _openssl_verify(name, q, digest, r, s) in (True, None)


def test_batcher_mixed_curves(gpu_ctx):
    from bftkv_amd import Batcher
    rng = np.random.default_rng(256)
    jobs = []
    for i in range(256):
        c = E.CURVES[E.NAMES[i % 4]]
        k = (2, 8, 3)[i % 3]
        xs, ri, vi = (v[0] for v in _random_ops(gpu_ctx, c, rng, 1, k)) if i < 8 else (v[0] for v in _identity_ops(gpu_ctx, c, rng, 1, k))
        if i == 17:
            ri = [ri[0], b"\x02" + ri[1][1:]] + ri[2:]            # this caller alone is fenced
        jobs.append((c, xs, ri, vi))
    want = [E.calculate_r(c, xs, ri, vi) if i < 8 or i == 17 else (E.OK, c["gx"] % c["n"]) for i, (c, xs, ri, vi) in enumerate(jobs)]
    assert want[17][0] == E.FENCED
    b = Batcher(gpu_ctx, max_items=64, n_lanes=2)
    got = [None] * 256

    def run(i):
        c, xs, ri, vi = jobs[i]
        got[i] = b.ecdsa_calculate_r(xs, ri, vi, c)

    th = [threading.Thread(target=run, args=(i,)) for i in range(256)]
    for t_ in th:
        t_.start()
    for t_ in th:
        t_.join()
    b.close()
    for i in range(256):
        assert got[i] == (0, *want[i]), i


def test_errors(gpu_ctx):
    from bftkv_amd._native import NativeError
    c = E.CURVES["P-256"]
    rng = np.random.default_rng(1)
    xs, ri, vi = _random_ops(gpu_ctx, c, rng, 2, 3)
    other = dict(c, b=c["b"] ^ 1)
    with pytest.raises(NativeError, match=r"\(-4\)"):
        gpu_ctx.ecdsa_calculate_r(xs, ri, vi, other)
    with pytest.raises(NativeError, match=r"\(-4\)"):
        gpu_ctx.ec_scalar_base_mult([1], other)
    with pytest.raises(NativeError, match=r"\(-4\)"):
        gpu_ctx.ecdsa_calculate_r(xs, ri, vi, dict(c, bit_size=255))
    lib, h = gpu_ctx.lib, gpu_ctx.h
    from bftkv_amd._native import _curve_bytes
    cb, bits, _ = _curve_bytes(c)
    buf = np.zeros(4096, dtype=np.uint8)
    P = lambda a: a.ctypes.data_as(C.c_void_p)        # noqa: E731
    assert lib.bftkv_gpu_ecdsa_calculate_r(h, 1, 0, P(buf), P(buf), P(buf), P(cb), bits, P(buf), P(buf)) == E_INVALID      # k = 0
    assert lib.bftkv_gpu_ecdsa_calculate_r(h, 1, 1025, P(buf), P(buf), P(buf), P(cb), bits, P(buf), P(buf)) == E_INVALID   # k > 1024
    assert lib.bftkv_gpu_ecdsa_calculate_r(h, 1, 2, None, P(buf), P(buf), P(cb), bits, P(buf), P(buf)) == E_INVALID
    assert lib.bftkv_gpu_ecdsa_calculate_r(h, 1, 2, P(buf), P(buf), P(buf), None, bits, P(buf), P(buf)) == E_INVALID
    assert lib.bftkv_gpu_ecdsa_calculate_r(None, 1, 2, P(buf), P(buf), P(buf), P(cb), bits, P(buf), P(buf)) == E_INVALID
    assert lib.bftkv_gpu_ecdsa_calculate_r(h, 0, 2, None, None, None, P(cb), bits, None, None) == 0
    assert lib.bftkv_gpu_ec_scalar_base_mult(h, 1, P(buf), 33, P(cb), bits, P(buf), P(buf)) == E_INVALID                 # sbytes > fbytes
    assert lib.bftkv_gpu_ec_scalar_base_mult(h, 1, P(buf), 0, P(cb), bits, P(buf), P(buf)) == E_INVALID
    st, out = np.zeros(1, dtype=np.uint8), np.full(32, 0xAA, dtype=np.uint8)
    assert lib.bftkv_gpu_batcher_ecdsa_calculate_r(None, 2, P(buf), P(buf), P(buf), P(cb), bits, P(out), P(st)) == E_INVALID
    assert st[0] == 0xFF and not out.any()
