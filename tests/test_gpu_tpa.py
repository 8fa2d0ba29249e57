"""GPU: the password-authentication entries (bftkv_gpu_tpa_yi / _bi / _ni and the batcher kinds) against the restatement
(tests/tpa_ref.py) over the seeded corpus (tests/tpa_cases.py), byte for byte."""
import ctypes as C
import threading

import numpy as np
import pytest

import tpa_cases as K
import tpa_ref as R

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED, OK, FAILED = -1, -4, 0, 0xFF
P8 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8))      # noqa: E731


def be_rows(vals, width):
    return np.frombuffer(b"".join(int(v).to_bytes(width, "big") for v in vals), dtype=np.uint8).reshape(len(vals), width).copy()


def front_rows(chunks, width):
    """each chunk at the front of its row; what follows is NOT zero (the entries must ignore it)"""
    a = np.full((len(chunks), width), 0xEE, dtype=np.uint8)
    for i, c in enumerate(chunks):
        a[i, :len(c)] = np.frombuffer(c, dtype=np.uint8)
    return a


def arrays(ops, nbytes=None, exp_len=None, kdf=True):
    """The call arrays of a list of ops: of one shape, or (kdf=False: no Xi, no salt) widened to nbytes and exp_len."""
    nbytes = nbytes or ops[0].nbytes
    exp_len = exp_len or ops[0].exp_len
    mods = sorted({op.p for op in ops})
    a = dict(v=be_rows([op.v for op in ops], nbytes), b=be_rows([op.b for op in ops], exp_len), mods=be_rows(mods, nbytes),
             mi=np.array([mods.index(op.p) for op in ops], dtype=np.uint32))
    if kdf:
        a.update(xi=front_rows([op.xi for op in ops], nbytes), xl=np.array([len(op.xi) for op in ops], dtype=np.uint32),
                 salt=front_rows([op.salt for op in ops], len(ops[0].salt)))
    return a


def want(idx, nbytes):
    exp = K.expected()
    yi = [exp[i][0].to_bytes(nbytes, "big") for i in idx]
    bi = [(exp[i][1][0].to_bytes(nbytes, "big"), exp[i][1][1], exp[i][1][2]) for i in idx]
    return yi, bi, [exp[i][2] for i in idx]


def odd_prefix(n):
    """a count below n that fills neither the last block's quads (64) with one chain per operation nor with two"""
    m = n - 1
    while m % 64 == 0 or (2 * m) % 64 == 0:
        m -= 1
    assert m > 0
    return m


def check_yi(ctx, idx, nbytes, exp_len):
    ops = [K.corpus()[i] for i in idx]
    a = arrays(ops, nbytes, exp_len, kdf=False)
    yi, st = ctx.tpa_yi(a["v"], a["b"], a["mods"], a["mi"])
    assert (st == OK).all()
    bad = [i for i, g, w in zip(idx, yi, want(idx, nbytes)[0]) if g.tobytes() != w]
    assert not bad, (len(bad), bad[:8], sorted(K.corpus()[bad[0]].tags))
    return a, yi


def test_yi_whole_corpus_in_one_shuffled_call(gpu_ctx):
    """every op widened to 256-byte numbers and exponents (leading zero bytes), in one call over every modulus of the corpus"""
    n = len(K.corpus())
    idx = [int(i) for i in np.random.default_rng(7).permutation(n)]
    check_yi(gpu_ctx, idx, 256, 256)
    check_yi(gpu_ctx, idx[:odd_prefix(n)], 256, 256)


def test_yi_equals_the_old_kernel(gpu_ctx):
    """k_modexp (square-and-always-multiply) on the same operands: same answers"""
    idx = list(range(0, len(K.corpus()), 3))
    a, yi = check_yi(gpu_ctx, idx, 256, 256)
    old = gpu_ctx.modexp_ops(a["v"], a["mi"], a["mods"], a["b"])
    assert (old == yi).all()


def test_more_chains_than_one_launch_takes(gpu_ctx):
    """k_tpa_pow goes out in launches of 65,536 chains on one table buffer: 66,001 short powers against the old kernel, all of them,
    and against pow() at both ends of every launch"""
    n = 66001
    rng = np.random.default_rng(66)
    mods = be_rows([R.P, K.moduli()["rsa2047"]], 256)
    x = rng.integers(0, 256, size=(n, 256), dtype=np.uint8)
    y = rng.integers(0, 256, size=(n, 8), dtype=np.uint8)
    mi = (np.arange(n) % 2).astype(np.uint32)
    yi, st = gpu_ctx.tpa_yi(x, y, mods, mi)
    assert (st == OK).all()
    assert (yi == gpu_ctx.modexp_ops(x, mi, mods, y)).all()
    for i in (0, 1, 65534, 65535, 65536, 65537, n - 2, n - 1):
        m = int.from_bytes(mods[mi[i]].tobytes(), "big")
        assert int.from_bytes(yi[i].tobytes(), "big") == pow(int.from_bytes(x[i].tobytes(), "big"), int.from_bytes(y[i].tobytes(), "big"), m), i


@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: "%d_%d_%d" % s)
def test_bi_and_ni_per_shape(gpu_ctx, shape):
    every = K.by_shape()[shape]
    for idx in (every, every[::-1][:odd_prefix(len(every))]):
        ops = [K.corpus()[i] for i in idx]
        a = arrays(ops)
        _, wbi, wni = want(idx, shape[0])
        bi, keys, mac, st = gpu_ctx.tpa_bi(a["v"], a["xi"], a["xl"], a["b"], a["salt"], a["mods"], a["mi"])
        assert (st == OK).all()
        bad = [(i, sorted(K.corpus()[i].tags)) for i, g, w in zip(idx, zip(bi, keys, mac), wbi) if tuple(x.tobytes() for x in g) != w]
        assert not bad, (len(bad), bad[:4])
        keys, ni, st = gpu_ctx.tpa_ni(a["v"], a["xi"], a["xl"], a["b"], a["salt"], a["mods"], a["mi"])
        assert (st == OK).all()
        bad = [(i, sorted(K.corpus()[i].tags)) for i, g, w in zip(idx, zip(keys, ni), wni) if tuple(x.tobytes() for x in g) != w]
        assert not bad, (len(bad), bad[:4])


def test_null_mod_idx_is_modulus_0_and_a_large_index_is_clamped(gpu_ctx):
    idx = [i for i in K.by_shape()[(256, 32, 16)] if K.corpus()[i].p == R.P][:5]
    a = arrays([K.corpus()[i] for i in idx])
    assert a["mods"].shape[0] == 1
    yi0, _ = gpu_ctx.tpa_yi(a["v"], a["b"], a["mods"], None)
    yi9, _ = gpu_ctx.tpa_yi(a["v"], a["b"], a["mods"], np.full(len(idx), 9, dtype=np.uint32))
    assert [y.tobytes() for y in yi0] == want(idx, 256)[0] == [y.tobytes() for y in yi9]


def test_the_device_closes_the_loop_on_the_honest_runs(gpu_ctx):
    """makeBi's answers go into processBi as they come off the device: every server's mac is the client's Ni, the keys agree"""
    mods = be_rows([R.P], 256)
    for run in K.honest_runs():
        sv = run["servers"]
        xi, xl = front_rows([s["xi"] for s in sv], 256), np.array([len(s["xi"]) for s in sv], dtype=np.uint32)
        salt = front_rows([s["salt"] for s in sv], 32)
        bi, skeys, mac, st = gpu_ctx.tpa_bi(be_rows([s["v"] for s in sv], 256), xi, xl, be_rows([s["b"] for s in sv], 256), salt, mods)
        assert (st == OK).all()
        ckeys, ni, st = gpu_ctx.tpa_ni(bi, xi, xl, be_rows([s["e"] for s in sv], 256), salt, mods)
        assert (st == OK).all()
        assert (mac == ni).all() and (skeys == ckeys).all()
        assert [m.tobytes() for m in mac] == [s["mac"] for s in sv] and [k.tobytes() for k in skeys] == [s["server_keys"] for s in sv]
        yi, st = gpu_ctx.tpa_yi(be_rows([int.from_bytes(run["X"], "big")] * len(sv), 256), be_rows([s["y"] for s in sv], 256), mods)
        assert [int.from_bytes(y.tobytes(), "big") for y in yi] == [s["yi"] for s in sv]


def test_a_changed_byte_changes_its_own_operation_alone(gpu_ctx):
    idx = [i for i in K.by_shape()[(256, 32, 16)] if len(K.corpus()[i].xi) > 8][:6]
    a = arrays([K.corpus()[i] for i in idx])
    call = lambda d: np.hstack(gpu_ctx.tpa_bi(d["v"], d["xi"], d["xl"], d["b"], d["salt"], d["mods"], d["mi"])[:3])      # noqa: E731  bi | keys | mac
    base = call(a)
    for op, field, col in ((1, "xi", 3), (2, "salt", 15), (4, "b", 31), (0, "b", 0)):
        d = {k: v.copy() for k, v in a.items()}
        d[field][op, col] ^= 0x40
        got = call(d)
        changed = [i for i in range(len(idx)) if (got[i] != base[i]).any()]
        assert changed == [op], (field, changed)
        assert (got[op, -32:] != base[op, -32:]).any(), field       # the MAC itself
    d = {k: v.copy() for k, v in a.items()}
    d["xi"][3, int(d["xl"][3]):] ^= 0xFF                              # bytes of the row past xi_len are not looked at
    assert (call(d) == base).all()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _raw_call(lib, h, entry, n=3, nb=256, el=32, sl=16, xi_len=7, n_mods=1, even=False, null=()):
    """A direct call with dirty result arrays -> (rc, status, [outputs]).  `null`: the arguments passed as NULL."""
    width = max(nb, 1)
    rng = np.random.default_rng(3)
    arr = lambda *shape: rng.integers(0, 256, size=shape, dtype=np.uint8)      # noqa: E731
    d = dict(base=arr(n or 1, width), xi=arr(n or 1, width), e=arr(n or 1, max(el, 1)), salt=arr(n or 1, max(sl, 1)),
             mods=be_rows([R.P - 1 if even else R.P], 256) if width == 256 else be_rows([(1 << (8 * width)) - 1 - (1 if even else 0)], width),
             xl=np.full(n or 1, xi_len, dtype=np.uint32), num=np.full((n or 1, width), 0xA5, dtype=np.uint8),
             keys=np.full((n or 1, 32), 0xA5, dtype=np.uint8), mac=np.full((n or 1, 32), 0xA5, dtype=np.uint8), st=np.zeros(n or 1, dtype=np.uint8))
    g = lambda k: None if k in null else (d[k].ctypes.data if k == "xl" else P8(d[k]))      # noqa: E731
    if entry == "yi":
        rc = lib.bftkv_gpu_tpa_yi(h, n, g("base"), nb, g("e"), el, None, n_mods, g("mods"), g("num"), g("st"))
        outs = ["num"]
    elif entry == "bi":
        rc = lib.bftkv_gpu_tpa_bi(h, n, g("base"), g("xi"), g("xl"), nb, g("e"), el, g("salt"), sl, None, n_mods, g("mods"), g("num"), g("keys"), g("mac"), g("st"))
        outs = ["num", "keys", "mac"]
    else:
        rc = lib.bftkv_gpu_tpa_ni(h, n, g("base"), g("xi"), g("xl"), nb, g("e"), el, g("salt"), sl, None, n_mods, g("mods"), g("keys"), g("mac"), g("st"))
        outs = ["keys", "mac"]
    d["num"] = d["num"].reshape(-1)[:(n or 1) * nb]                  # the bytes the call was told the rows have
    return rc, d["st"], [d[k] for k in outs if k not in null]


REFUSALS = [dict(nb=0), dict(nb=257), dict(el=0), dict(el=257), dict(n_mods=0), dict(n=0), dict(null=("base",)), dict(null=("e",)),
            dict(null=("mods",))]
KDF_REFUSALS = [dict(sl=65), dict(xi_len=257), dict(nb=128, xi_len=129), dict(null=("xi",)), dict(null=("xl",)), dict(null=("salt",)),
                dict(null=("keys",)), dict(null=("mac",))]


@pytest.mark.parametrize("entry", ["yi", "bi", "ni"])
def test_refusals_of_the_direct_entries(gpu_ctx, entry):
    lib, h = gpu_ctx.lib, gpu_ctx.h
    rows = REFUSALS + (KDF_REFUSALS if entry != "yi" else []) + ([dict(null=("num",))] if entry != "ni" else [])
    for kw in rows:
        rc, st, outs = _raw_call(lib, h, entry, **kw)
        assert rc == E_INVALID, (entry, kw, rc)
        if kw.get("n", 3):
            assert (st == FAILED).all() and all(not o.any() for o in outs), (entry, kw)
    rc, st, outs = _raw_call(lib, h, entry, even=True)
    assert rc == E_UNSUPPORTED and (st == FAILED).all() and all(not o.any() for o in outs)
    rc, st, outs = _raw_call(lib, None, entry)
    assert rc == E_INVALID and (st == FAILED).all() and all(not o.any() for o in outs)
    rc, st, outs = _raw_call(lib, h, entry, sl=0, null=("salt",))     # no salt at all is a call like any other
    assert rc == 0 and (st == OK).all() and all(o.any() for o in outs)
    rc, st, outs = _raw_call(lib, h, entry)
    assert rc == 0 and (st == OK).all() and all(o.any() for o in outs)


def test_refusals_of_the_batcher_entries(gpu_ctx):
    """a refused caller gets its error alone, before it joins a batch: the valid callers beside it get their answers"""
    from bftkv_amd import Batcher
    idx = [i for i in K.by_shape()[(256, 32, 16)] if K.corpus()[i].xi][:4]
    ops = [K.corpus()[i] for i in idx]
    _, wbi, _ = want(idx, 256)
    b = Batcher(gpu_ctx, max_items=16, max_wait_us=2000, n_lanes=1)
    pb = lambda v, w=256: int(v).to_bytes(w, "big")      # noqa: E731
    op = ops[0]
    good = dict(v=pb(op.v), xi=op.xi, b=pb(op.b, 32), salt=op.salt, mod=pb(op.p))
    bad_rows = [dict(v=b"", mod=b""), dict(v=pb(1, 257), mod=pb(3, 257)), dict(b=b""), dict(b=pb(1, 257)), dict(salt=b"s" * 65),
                dict(v=pb(op.v % (1 << 1024), 128), mod=pb(op.p % (1 << 1024) | 1, 128), xi=b"x" * 129)]
    res, refused = {}, {}

    def valid(j):
        o = ops[j]
        res[j] = b.tpa_bi(pb(o.v), o.xi, pb(o.b, 32), o.salt, pb(o.p))

    def bad(j):
        refused[j] = b.tpa_bi(**dict(good, **bad_rows[j]))

    th = [threading.Thread(target=valid, args=(j,)) for j in range(len(ops))] + [threading.Thread(target=bad, args=(j,)) for j in range(len(bad_rows))]
    for t_ in th:
        t_.start()
    for t_ in th:
        t_.join()
    for j in range(len(ops)):
        assert res[j] == (0, OK) + wbi[j], j
    for j, r in refused.items():
        assert r[:2] == (E_INVALID, FAILED) and not any(r[2]) and not any(r[3]) and not any(r[4]), (j, r[:2])
    r = b.tpa_bi(**dict(good, mod=pb(op.p - 1)))
    assert r[:2] == (E_UNSUPPORTED, FAILED) and not any(r[2] + r[3] + r[4])
    r = b.tpa_yi(pb(op.v), pb(op.b, 32), pb(op.p - 1))
    assert r[:2] == (E_UNSUPPORTED, FAILED) and not any(r[2])
    for kw in (dict(x=b"", mod=b""), dict(y=b""), dict(y=pb(1, 257)), dict(x=pb(1, 257), mod=pb(3, 257))):
        r = b.tpa_yi(**dict(dict(x=pb(op.v), y=pb(op.b, 32), mod=pb(op.p)), **kw))
        assert r[:2] == (E_INVALID, FAILED) and not any(r[2]), kw
    # NULL arrays and a NULL batcher, through the library itself
    lib = gpu_ctx.lib
    v, e, m = be_rows([op.v], 256), be_rows([op.b], 32), be_rows([op.p], 256)
    out, st = np.full(256, 0xA5, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
    for args in ((None, P8(v), 256, P8(e), 32, P8(m)), (b.h, None, 256, P8(e), 32, P8(m)), (b.h, P8(v), 256, None, 32, P8(m)),
                 (b.h, P8(v), 256, P8(e), 32, None)):
        out[:], st[0] = 0xA5, 0
        assert lib.bftkv_gpu_batcher_tpa_yi(*args, P8(out), P8(st)) == E_INVALID and st[0] == FAILED and not out.any()
    assert b.tpa_yi(pb(op.v), pb(op.b, 32), pb(op.p)) == (0, OK, want(idx[:1], 256)[0][0])
    b.close()


def test_64_threads_through_the_batcher(gpu_ctx):
    from bftkv_amd import Batcher
    pool = K.by_shape()[(256, 32, 16)]
    names = sorted({t for i in pool for t in K.corpus()[i].tags if t.startswith("mod:")})[:4]
    few = [i for i in pool if K.corpus()[i].tags & set(names)]
    idx = [few[j % len(few)] for j in range(64)]
    assert len(few) >= 8 and len({K.corpus()[i].p for i in idx}) == 4
    yi, wbi, _ = want(idx, 256)
    pb = lambda v, w=256: int(v).to_bytes(w, "big")      # noqa: E731
    for kind in ("bi", "yi"):
        b = Batcher(gpu_ctx, max_items=64, max_wait_us=5000, n_lanes=2)
        got = [None] * 64
        gate = threading.Barrier(64)

        def run(j):
            o = K.corpus()[idx[j]]
            gate.wait()
            got[j] = b.tpa_bi(pb(o.v), o.xi, pb(o.b, 32), o.salt, pb(o.p)) if kind == "bi" else b.tpa_yi(pb(o.v), pb(o.b, 32), pb(o.p))

        th = [threading.Thread(target=run, args=(j,)) for j in range(64)]
        for t_ in th:
            t_.start()
        for t_ in th:
            t_.join()
        stats = b.stats()
        b.close()
        for j in range(64):
            assert got[j] == ((0, OK) + wbi[j] if kind == "bi" else (0, OK, yi[j])), (kind, j)
        assert stats["calls"] == 64 and stats["batches"] < 64 and stats["max_batch"] > 1, stats
