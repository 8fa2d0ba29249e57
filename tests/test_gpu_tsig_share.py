"""-m gpu: threshold DSA / ECDSA signing, the server's share answers (bftkv_gpu_tdsa_share, bftkv_gpu_tecdsa_share, bftkv_gpu_tsig_partial_s,
their _dev forms and the two batcher kinds), byte for byte against the restatement (tests/tsig_share_ref.py) over the seeded corpus
(tests/tsig_share_cases.py).  Every status is OK: the corpus holds no other, and every test asserts it.  Shapes are the smallest at which
the kernels can still go wrong: every ai and sum class once, the quad-per-wave and block boundaries, one wave of sixteen digit patterns."""
import functools
import threading

import numpy as np
import pytest

import ec_ref as E
import tsig_share_cases as K
import tsig_share_ref as R

pytestmark = pytest.mark.gpu
E_INVALID, E_UNSUPPORTED = -1, -4
GUARD = 0x5A


def _be(v, w):
    return np.frombuffer(int(v).to_bytes(w, "big"), dtype=np.uint8)


def _dsa_want(g, pb, qb, reqs):
    G = R.dsa_group(g.p, g.q, g.g, pb, qb)
    out = [R.phase2(G, sh) for sh in reqs]
    return (b"".join(a.ri for a in out), b"".join(a.vi.to_bytes(qb, "big") for a in out), b"".join(a.ki.to_bytes(qb, "big") for a in out),
            b"".join(a.ci.to_bytes(qb, "big") for a in out))


@functools.lru_cache(maxsize=None)
def _ec_ri(name, ai):
    return E.calculate_partial_r(E.CURVES[name], ai)


def _ec_want(name, reqs):
    c = E.CURVES[name]
    f, n = E.byte_len(c), c["n"]
    out = []
    for sh in reqs:
        ki, ai, bi, ci = R.fold(sh, n)
        out.append(R.Answer(ki, ai, bi, ci, _ec_ri(name, ai), R.vi_of(n, ki, ai, bi)))
    return (b"".join(a.ri for a in out), b"".join(a.vi.to_bytes(f, "big") for a in out), b"".join(a.ki.to_bytes(f, "big") for a in out),
            b"".join(a.ci.to_bytes(f, "big") for a in out))


def _check(got, want, labels, what):
    ri, vi, ki, ci, st = got
    assert not st.any(), (what, [int(s) for s in st])                       # every status OK
    n = len(st)
    for name, g, w in zip(("ri", "vi", "ki", "ci"), (ri, vi, ki, ci), want):
        g = g.tobytes()
        if g != w:
            width = len(w) // n
            bad = [labels[i] for i in range(n) if g[i * width:(i + 1) * width] != w[i * width:(i + 1) * width]]
            raise AssertionError((what, name, bad[:8], len(bad)))


@pytest.fixture(scope="module")
def dsa_sets(gpu_ctx):
    """sets of one group each at window widths 4, 5 and 8, and one set of both groups at the default width; one key y each"""
    made = {}
    gs = K.dsa_groups()
    for name, g in gs.items():
        for w in (4, 5, 8):
            made[(name, w)] = gpu_ctx.dsa_keyset_create([(0, g.y)], [(g.p, g.q, g.g)], window_bits=w)
    both = [gs["dsa1024"], gs["dsa2048"]]
    made["both"] = gpu_ctx.dsa_keyset_create([(0, both[0].y), (1, both[1].y)], [(g.p, g.q, g.g) for g in both], pbytes=256, qbytes=32)
    yield made
    for h in made.values():
        gpu_ctx.dsa_keyset_destroy(h)


# ---- DSA ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [4, 5, 8])
@pytest.mark.parametrize("gname", K.DSA_NAMES)
def test_dsa_every_class(gpu_ctx, dsa_sets, gname, w):
    g = K.dsa_groups()[gname]
    ks = dsa_sets[(gname, w)]
    info = gpu_ctx.dsa_keyset_info(ks)
    pb, qb = info["pbytes"], info["qbytes"]
    assert info["window_bits"] == w and info["windows"] == K.windows_of(g.q, w) and (w != 5 or 28 % w)      # 5 divides no limb: digits straddle
    for m in (1, 2, 4, 7):
        cases = K.requests(g.q, qb, m, w, info["windows"], seed=m)
        labels, reqs = [lb for lb, _ in cases], [sh for _, sh in cases]
        assert {"s:" + c for c in K.SUM_CLASSES} <= set(labels) and "a:zero" in labels and sum(lb.startswith("a:digit@") for lb in labels) >= info["windows"] - 1
        got = gpu_ctx.tdsa_share(ks, K.shares_array(reqs, qb))
        _check(got, _dsa_want(g, pb, qb, reqs), labels, (gname, w, m))
        zero = labels.index("a:zero")
        assert int.from_bytes(got[0][zero].tobytes(), "big") == 1                   # ai = 0: ri = 1
        above = labels.index("s:above_q")
        assert all(v >= g.q for tup in reqs[above] for v in tup)


def test_dsa_both_groups_mixed_inside_a_wave(gpu_ctx, dsa_sets):
    """a 160-bit q in 32-byte rows beside a 256-bit one; group_idx alternates inside every wave, and an index past the set is clamped"""
    gs = [K.dsa_groups()[n] for n in K.DSA_NAMES]
    ks = dsa_sets["both"]
    info = gpu_ctx.dsa_keyset_info(ks)
    assert (info["pbytes"], info["qbytes"], info["window_bits"], info["n_groups"]) == (256, 32, 8, 2)
    assert gs[0].q.bit_length() == 160 and gs[1].q.bit_length() == 256
    per = [K.requests(g.q, 32, 2, 8, K.windows_of(g.q, 8), seed=9) for g in gs]
    n = min(len(per[0]), len(per[1]))
    pattern = [(i * 7 // 3) % 2 for i in range(2 * n)]
    idx, reqs, labels, want = [], [], [], [[], [], [], []]
    at = [0, 0]
    for gi in pattern:
        if at[gi] >= n:
            gi ^= 1
        lb, sh = per[gi][at[gi]]
        at[gi] += 1
        idx.append(gi if len(idx) % 5 else gi * 77)              # 77: clamped to group 1
        reqs.append(sh)
        labels.append("g%d:%s" % (gi, lb))
        for k, part in enumerate(_dsa_want(gs[gi], 256, 32, [sh])):
            want[k].append(part)
    assert len({i for i in idx[:16]}) > 1
    got = gpu_ctx.tdsa_share(ks, K.shares_array(reqs, 32), group_idx=idx)
    _check(got, [b"".join(w) for w in want], labels, "both groups")


def _dev_share(gpu_ctx, call, shares, ri_w, q_w):
    """a _dev call with guard bytes behind every output -> (ri, vi, ki, ci, st) and the guards' bytes"""
    import torch
    n = shares.shape[0]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")    # noqa: E731
    d_sh = up(shares.reshape(-1))
    outs = [torch.full((n * w + 64,), GUARD, dtype=torch.uint8, device="cuda:0") for w in (ri_w, q_w, q_w, q_w, 1)]
    gpu_ctx._check(call(n, shares.shape[1], d_sh.data_ptr(), *[o.data_ptr() for o in outs]), "share_dev")
    gpu_ctx.sync()
    host = [o.cpu().numpy() for o in outs]
    body = [h[:n * w].reshape(n, w) if w > 1 else h[:n] for h, w in zip(host, (ri_w, q_w, q_w, q_w, 1))]
    guards = b"".join(h[n * w:].tobytes() for h, w in zip(host, (ri_w, q_w, q_w, q_w, 1)))
    return body, guards


@pytest.mark.parametrize("n", [1, 15, 16, 17, 65])
def test_dsa_dev_form_at_the_wave_and_block_boundaries(gpu_ctx, dsa_sets, n):
    """16 quads make a wave, 64 a block: the padding lane groups store nothing (the guard bytes behind every output stay)"""
    import torch
    g = K.dsa_groups()["dsa2048"]
    ks = dsa_sets[("dsa2048", 8)]
    cases = K.requests(g.q, 32, 4, 8, 32, seed=n)[:n]
    labels, reqs = [lb for lb, _ in cases], [sh for _, sh in cases]
    sh = K.shares_array(reqs, 32)
    lib, h = gpu_ctx.lib, gpu_ctx.h
    d_gi = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    for gi_ptr in (None, d_gi.data_ptr()):
        body, guards = _dev_share(gpu_ctx, lambda nn, m, s, ri, vi, ki, ci, st: lib.bftkv_gpu_tdsa_share_dev(h, ks, nn, gi_ptr, m, s, ri, vi, ki, ci, st), sh, 256, 32)
        _check(body, _dsa_want(g, 256, 32, reqs), labels, ("dev", n))
        assert guards == bytes([GUARD]) * len(guards)
    host = gpu_ctx.tdsa_share(ks, sh)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(host, body))


def test_dsa_sixteen_digit_patterns_in_one_wave(gpu_ctx, dsa_sets):
    g = K.dsa_groups()["dsa2048"]
    q = g.q
    pats = [0, 1, q - 1, (1 << 256) - 1, 1 << 248, 0xFF, 0xFF << 248 if (0xFF << 248) < q else 1 << 255, int("01" * 32, 16), int("00ff" * 16, 16), int("ff00" * 16, 16) % q,
            int("80" * 32, 16) % q, 1 << 128, (1 << 128) - 1, q - 2, q >> 1, 0x0100]
    assert len(set(p % q for p in pats)) == 16
    reqs = [[(3, p, 5, 7)] for p in pats]
    for w in (4, 5, 8):
        got = gpu_ctx.tdsa_share(dsa_sets[("dsa2048", w)], K.shares_array(reqs, 32))
        _check(got, _dsa_want(g, 256, 32, reqs), ["pat%d" % i for i in range(16)], ("patterns", w))


# ---- ECDSA ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.NAMES)
def test_ecdsa_every_class(gpu_ctx, name):
    c = E.CURVES[name]
    f, n = E.byte_len(c), c["n"]
    nwin = (8 * f + 3) // 4
    for m in (2, 1, 4, 7):
        cases = K.requests(n, f, m, 4, nwin, seed=m)
        if m != 2:                                   # every class once at m = 2; the sum classes and a few scalars at the other counts
            cases = [cs for cs in cases if cs[0].startswith("s:") or cs[0] in ("a:zero", "a:one", "a:q_minus_1", "a:all_max", "a:random0")]
        labels, reqs = [lb for lb, _ in cases], [sh for _, sh in cases]
        got = gpu_ctx.tecdsa_share(K.shares_array(reqs, f), c)
        _check(got, _ec_want(name, reqs), labels, (name, m))
        zero = labels.index("a:zero")
        assert got[0][zero].tobytes() == b"\x04" + bytes(2 * f)                     # ai = 0: Marshal of (0, 0)
        if m == 2:
            assert {"s:" + k for k in K.SUM_CLASSES} <= set(labels) and sum(lb.startswith("a:digit@") for lb in labels) >= (n.bit_length() - 1) // 4


@pytest.mark.parametrize("n_reqs", [1, 63, 64, 65])
@pytest.mark.parametrize("name", E.NAMES)
def test_ecdsa_dev_form_at_the_block_boundaries(gpu_ctx, name, n_reqs):
    c = E.CURVES[name]
    f, n = E.byte_len(c), c["n"]
    cases = K.requests(n, f, 2, 4, (8 * f + 3) // 4, seed=2)[:n_reqs]      # (the scalars of test_ecdsa_every_class: their points are remembered)
    labels, reqs = [lb for lb, _ in cases], [sh for _, sh in cases]
    sh = K.shares_array(reqs, f)
    from bftkv_amd._native import _curve_bytes, _ptr
    cb, bits, _ = _curve_bytes(c)
    lib, h = gpu_ctx.lib, gpu_ctx.h
    body, guards = _dev_share(gpu_ctx, lambda nn, m, s, ri, vi, ki, ci, st: lib.bftkv_gpu_tecdsa_share_dev(h, nn, m, s, _ptr(cb), bits, ri, vi, ki, ci, st), sh, 1 + 2 * f, f)
    _check(body, _ec_want(name, reqs), labels, ("dev", name, n_reqs))
    assert guards == bytes([GUARD]) * len(guards)
    host = gpu_ctx.tecdsa_share(sh, c)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(host, body))


# ---- phase 3 ----------------------------------------------------------------------------------------------------------------------------------
def test_partial_s_under_orders_of_20_28_32_and_66_bytes(gpu_ctx):
    mods = [(20, K.dsa_groups()["dsa1024"].q), (28, E.CURVES["P-224"]["n"]), (32, K.dsa_groups()["dsa2048"].q), (32, E.CURVES["P-256"]["n"]),
            (66, E.CURVES["P-521"]["n"])]
    for nb, q in mods:
        assert (q.bit_length() + 7) // 8 == nb
        cases = K.s_cases(q, nb)
        assert {"edge0", "edge4", "all_edge", "inner_on_q", "outer_on_q", "all_above"} <= {cs[0] for cs in cases}
        rows = lambda j: np.stack([_be(cs[j], nb) for cs in cases])      # noqa: E731
        si, st = gpu_ctx.tsig_partial_s(rows(1), rows(2), rows(3), rows(4), rows(5), _be(q, nb).reshape(1, nb))
        assert not st.any()
        want = [R.phase3(q, r, y, m, k, c) for _, m, r, y, k, c in cases]
        bad = [cs[0] for cs, s, w in zip(cases, si, want) if int.from_bytes(s.tobytes(), "big") != w]
        assert not bad, (nb, bad)
    # two orders in one call, an index past the table clamped to its last row
    q0, q1 = mods[2][1], mods[3][1]
    cs = K.s_cases(q0, 32)[:12]
    idx = [i % 2 if i % 5 else 9 for i in range(12)]
    rows = lambda j: np.stack([_be(c[j], 32) for c in cs])      # noqa: E731
    si, st = gpu_ctx.tsig_partial_s(rows(1), rows(2), rows(3), rows(4), rows(5), np.stack([_be(q0, 32), _be(q1, 32)]), mod_idx=idx)
    assert not st.any()
    assert [int.from_bytes(s.tobytes(), "big") for s in si] == [R.phase3(q1 if i else q0, r, y, m, k, c) for i, (_, m, r, y, k, c) in zip(idx, cs)]


# ---- the batcher and the refusals -----------------------------------------------------------------------------------------------------------------
def test_32_threads_through_the_batcher(gpu_ctx, dsa_sets):
    """both kinds, m of 1, 2, 4 and 7, two curves and two groups of one set: everybody gets the direct entry's bytes; a caller with m = 0
    is refused alone"""
    from bftkv_amd import Batcher
    gs = [K.dsa_groups()[n] for n in K.DSA_NAMES]
    ks = dsa_sets["both"]
    callers, direct = [], []
    for j in range(32):
        m = (1, 2, 4, 7)[j % 4]
        if j % 2:
            gi = (j // 2) % 2
            sh = K.requests(gs[gi].q, 32, m, 8, 32, seed=100 + j)[6 + j][1]
            callers.append(("dsa", gi, sh, m))
            got = gpu_ctx.tdsa_share(ks, K.shares_array([sh], 32), group_idx=[gi])
            _check(got, _dsa_want(gs[gi], 256, 32, [sh]), ["caller%d" % j], j)
        else:
            name = ("P-256", "P-384")[(j // 2) % 2]
            c = E.CURVES[name]
            f = E.byte_len(c)
            sh = K.requests(c["n"], f, m, 4, 2 * f, seed=100 + j)[j % 6][1]
            callers.append(("ec", name, sh, m))
            got = gpu_ctx.tecdsa_share(K.shares_array([sh], f), c)
            _check(got, _ec_want(name, [sh]), ["caller%d" % j], j)
        direct.append((0, 0) + tuple(a[0].tobytes() for a in got[:4]))
    b = Batcher(gpu_ctx, max_items=32, max_wait_us=5000, n_lanes=2)
    got = [None] * 32
    gate = threading.Barrier(32)

    def run(j):
        kind, which, sh, m = callers[j]
        gate.wait()
        if j == 13:                                                       # an argument error of one caller: m = 0
            got[j] = b.tdsa_share(ks, which, np.zeros((0, 4, 32), dtype=np.uint8))
        elif kind == "dsa":
            got[j] = b.tdsa_share(ks, which, K.shares_array([sh], 32)[0])
        else:
            got[j] = b.tecdsa_share(K.shares_array([sh], E.byte_len(E.CURVES[which]))[0], E.CURVES[which])

    th = [threading.Thread(target=run, args=(j,)) for j in range(32)]
    for t_ in th:
        t_.start()
    for t_ in th:
        t_.join()
    stats = b.stats()
    for j in range(32):
        if j == 13:
            assert got[j][0] == E_INVALID and got[j][1] == R.FAILED and not any(any(x) for x in got[j][2:]), j
        else:
            assert got[j] == direct[j], j
    assert stats["calls"] == 31 and stats["batches"] < 31 and stats["max_batch"] > 1, stats
    # refused for the caller alone, before it joins a batch: a bad handle, widths that are not the set's, an unrecognised curve
    one = K.shares_array([callers[1][2]], 32)[0]
    rc, st, *outs = b.tdsa_share(ks, 0, one)
    assert rc == 0 and st == 0
    lib = gpu_ctx.lib
    from bftkv_amd._native import _ptr
    for handle, pb in ((9999, 256), (ks, 128)):
        ri, vi, ki, ci, s1 = (np.full(w, 0xA5, dtype=np.uint8) for w in (pb, 32, 32, 32, 1))
        rc = lib.bftkv_gpu_batcher_tdsa_share(b.h, handle, 0, one.shape[0], _ptr(one), pb, 32, _ptr(ri), _ptr(vi), _ptr(ki), _ptr(ci), _ptr(s1))
        assert rc == E_INVALID and s1[0] == R.FAILED and not any(a.any() for a in (ri, vi, ki, ci)), handle
    bad = dict(E.CURVES["P-256"], b=E.CURVES["P-256"]["b"] ^ 1)
    rc, st, *outs = b.tecdsa_share(K.shares_array([callers[0][2]], 32)[0], bad)
    assert rc == E_UNSUPPORTED and st == R.FAILED and not any(any(x) for x in outs)
    b.close()


def test_refusals_of_the_direct_entries(gpu_ctx, dsa_sets):
    lib, h = gpu_ctx.lib, gpu_ctx.h
    from bftkv_amd._native import _curve_bytes, _ptr
    ks = dsa_sets[("dsa2048", 8)]
    sh = np.full((3, 2, 4, 32), 0x11, dtype=np.uint8)
    dirty = lambda *shape: np.full(shape, 0xA5, dtype=np.uint8)      # noqa: E731

    def tdsa(handle, n, m, shares=sh, null_out=False):
        ri, vi, ki, ci, st = dirty(3, 256), dirty(3, 32), dirty(3, 32), dirty(3, 32), np.zeros(3, dtype=np.uint8)
        rc = lib.bftkv_gpu_tdsa_share(h, handle, n, None, m, None if shares is None else _ptr(shares), None if null_out else _ptr(ri), _ptr(vi), _ptr(ki), _ptr(ci), _ptr(st))
        return rc, st, (ri, vi, ki, ci)
    rc, st, outs = tdsa(ks, 3, 2)
    assert rc == 0 and not st.any() and all(o.any() for o in outs)
    for what, args in (("m = 0", (ks, 3, 0)), ("m > 1024", (ks, 3, 1025)), ("no shares", (ks, 3, 2, None)), ("a NULL output", (ks, 3, 2, sh, True))):
        rc, st, outs = tdsa(*args)
        assert rc == E_INVALID and (st == R.FAILED).all() and not any(o.any() for o in outs[1:]), what
    rc, st, outs = tdsa(4242, 3, 2)                                         # a bad handle: the widths are unknown, the statuses fail
    assert rc == E_INVALID and (st == R.FAILED).all()
    st0 = np.zeros(3, dtype=np.uint8)
    assert lib.bftkv_gpu_tdsa_share(h, ks, 0, None, 2, _ptr(sh), _ptr(dirty(1)), _ptr(dirty(1)), _ptr(dirty(1)), _ptr(dirty(1)), _ptr(st0)) == E_INVALID

    c = E.CURVES["P-256"]

    def tec(curve, bits, n, m):
        cb = _curve_bytes(dict(curve, bit_size=256))[0]
        ri, vi, ki, ci, st = dirty(3, 65), dirty(3, 32), dirty(3, 32), dirty(3, 32), np.zeros(3, dtype=np.uint8)
        rc = lib.bftkv_gpu_tecdsa_share(h, n, m, _ptr(sh), _ptr(cb), bits, _ptr(ri), _ptr(vi), _ptr(ki), _ptr(ci), _ptr(st))
        return rc, st, (ri, vi, ki, ci)
    rc, st, outs = tec(c, 256, 3, 2)
    assert rc == 0 and not st.any()
    for what, want, args in (("an unrecognised curve", E_UNSUPPORTED, (dict(c, gx=c["gx"] ^ 2), 256, 3, 2)), ("m = 0", E_INVALID, (c, 256, 3, 0)),
                             ("m > 1024", E_INVALID, (c, 256, 3, 1025))):
        rc, st, outs = tec(*args)
        assert rc == want and (st == R.FAILED).all() and not any(o.any() for o in outs), what
    rc, st, outs = tec(c, 522, 3, 2)
    assert rc == E_INVALID

    q = E.CURVES["P-256"]["n"]
    a = [dirty(3, 32) for _ in range(5)]

    def ps(qq, nb=32, n_mods=1):
        si, st = dirty(3, 32), np.zeros(3, dtype=np.uint8)
        rc = lib.bftkv_gpu_tsig_partial_s(h, 3, *[_ptr(x) for x in a], nb, None, n_mods, _ptr(np.ascontiguousarray(_be(qq, 32))), _ptr(si), _ptr(st))
        return rc, st, si
    rc, st, si = ps(q)
    assert rc == 0 and not st.any()
    for what, want, kw in (("an even q", E_UNSUPPORTED, dict(qq=q - 1)), ("q = 0", E_UNSUPPORTED, dict(qq=0)), ("no moduli", E_INVALID, dict(qq=q, n_mods=0))):
        rc, st, si = ps(**kw)
        assert rc == want and (st == R.FAILED).all() and not si.any(), what
    si, st = dirty(3, 67), np.zeros(3, dtype=np.uint8)
    wide = [dirty(3, 67) for _ in range(5)]
    assert lib.bftkv_gpu_tsig_partial_s(h, 3, *[_ptr(x) for x in wide], 67, None, 1, _ptr(dirty(67)), _ptr(si), _ptr(st)) == E_INVALID
