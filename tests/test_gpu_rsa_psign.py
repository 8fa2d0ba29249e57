"""GPU: threshold RSA signing, the server's side (bftkv_gpu_rsa_partial_sign and the batcher kind) against the restatement
(tests/rsa_psign_ref.py) over the seeded corpus (tests/rsa_psign_cases.py): byte for byte and status for status, no sampling."""
import ctypes as C
import hashlib
import os
import random
import threading

import numpy as np
import pytest

import rsa_psign_cases as K
import rsa_psign_ref as R

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -4
TPA_LAUNCH_CHAINS = 1 << 16                                         # bftkv_amd/csrc/tpa_capi.inc
P8 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8))      # noqa: E731
A32 = lambda a: None if a is None else a.ctypes.data                               # noqa: E731


def be_rows(vals, width):
    return np.frombuffer(b"".join(int(v).to_bytes(width, "big") for v in vals), dtype=np.uint8).reshape(len(vals), width).copy()


def sign_call(ctx, reqs, frags, nbytes, exp_len, used=True):
    """reqs [(n, T)], frags [(request, sign byte, magnitude, exp_used)] -> (out, status) of ONE call; used=False: no exp_used array"""
    mods = sorted({n for n, _ in reqs})
    t_cap = max(len(t) for _, t in reqs)
    t = np.full((len(reqs), t_cap), 0xEE, dtype=np.uint8)
    for i, (_, tt) in enumerate(reqs):
        t[i, :len(tt)] = np.frombuffer(tt, dtype=np.uint8)
    return ctx.rsa_partial_sign(t, [len(tt) for _, tt in reqs], be_rows(mods, nbytes), be_rows([f[2] for f in frags], exp_len), [f[1] for f in frags],
                                mod_idx=[mods.index(n) for n, _ in reqs], frag_req=[f[0] for f in frags], exp_used=[f[3] for f in frags] if used else None)


def want_rows(reqs, frags, nbytes):
    """the restatement's (status, bytes) per fragment"""
    out = []
    for r, sb, mag, _ in frags:
        st, ci = R.sign(reqs[r][1], reqs[r][0], [(sb, mag)])[0]
        out.append((st, ci.to_bytes(nbytes, "big")))
    return out


def assert_rows(out, st, want, what=""):
    bad = [i for i, (s, b) in enumerate(want) if int(st[i]) != s or out[i].tobytes() != b]
    assert not bad, (what, len(bad), bad[:8], [(int(st[i]), want[i][0]) for i in bad[:8]])


# ---- 1. the corpus, one call per shape ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(K.calls())), ids=[c.name for c in K.calls()])
def test_corpus_in_one_call(gpu_ctx, ci):
    call = K.calls()[ci]
    want = [(s, v.to_bytes(call.nbytes, "big")) for s, v in K.expected(ci)]
    n = len(want)
    for order in (list(range(n)), [int(i) for i in np.random.default_rng(ci).permutation(n)]):
        a = K.call_arrays(call, order)
        out, st = gpu_ctx.rsa_partial_sign(a["t"], a["t_len"], a["mods"], a["exps"], a["sign"], a["mod_idx"], a["frag_req"], a["exp_used"])
        assert_rows(out, st, [want[j] for j in order], call.name)
    assert {s for s, _ in want} >= ({R.OK} if call.exp_len == K.BIG_EXP_LEN else {R.OK, R.INVALID_INPUT})


def test_no_inverse_beside_its_siblings(gpu_ctx):
    """N = 3 P with 3 | em: the negative fragment has no answer, its non-negative siblings have theirs; a coprime T under the same N is all OK"""
    n3, t_bad, t_good = K.no_inverse_case()
    reqs = [(n3, t_bad), (n3, t_good), (K.kat()["n"], t_bad)]
    frags = [(r, sb, mag, 5) for r in range(3) for sb, mag in ((1, 0x1234567), (0, 0x1234567), (0xFF, 0), (2, 1), (0, 0))]
    out, st = sign_call(gpu_ctx, reqs, frags, 256, 5)
    assert_rows(out, st, want_rows(reqs, frags, 256))
    assert [int(s) for s in st] == [R.NO_INVERSE, 0, 0, R.NO_INVERSE, 0] + [0] * 10 and not out[0].any() and not out[3].any()


def test_null_arrays_that_are_optional_and_clamped_indices(gpu_ctx):
    k = K.kat()
    t = K.tree_t()
    frags = [(0, 1, 0xABCDEF, 3), (0, 0, 0x0102, 3), (0, 2, 0, 3)]
    want = want_rows([(k["n"], t)], frags, 256)
    tt = np.frombuffer(t, dtype=np.uint8).reshape(1, -1)
    mods, exps, sg = be_rows([k["n"]], 256), be_rows([f[2] for f in frags], 3), [f[1] for f in frags]
    for kw in (dict(), dict(mod_idx=[7], frag_req=[9, 9, 9]), dict(exp_used=[3, 2, 0])):
        out, st = gpu_ctx.rsa_partial_sign(tt, [len(t)], mods, exps, sg, **kw)
        assert_rows(out, st, want, str(kw))
    out, st = gpu_ctx.rsa_partial_sign(np.zeros((1, 0), dtype=np.uint8), [0], mods, exps, sg)      # t_cap 0: no T array at all
    assert_rows(out, st, want_rows([(k["n"], b"")], frags, 256), "empty T")


def test_a_modulus_of_zero_refuses_its_requests_alone(gpu_ctx):
    k = K.kat()
    reqs = [(0, b"\1\2"), (k["n"], b"\1\2"), (0, b"")]
    frags = [(0, 0, 5, 1), (1, 1, 5, 1), (1, 0, 5, 1), (2, 1, 0, 1)]
    out, st = sign_call(gpu_ctx, reqs, frags, 256, 1)
    assert_rows(out, st, want_rows(reqs, frags, 256))
    assert [int(s) for s in st] == [R.INVALID_INPUT, 0, 0, R.INVALID_INPUT]


# ---- 2. the loop closes on the device -------------------------------------------------------------------------------------------------------
def _tree_call(ctx, flip=None):
    """every fragment of every server of the n = 4, k = 2 tree in ONE call -> {(server, kid): ci}"""
    k = K.kat()
    fr = K.tree_fragments()
    exp_len = max(len(f[3]) for f in fr)
    exps = np.zeros((len(fr), exp_len), dtype=np.uint8)
    for i, f in enumerate(fr):
        exps[i, exp_len - len(f[3]):] = np.frombuffer(f[3], dtype=np.uint8)
    if flip is not None:
        exps[flip, exp_len - 7] ^= 0x10
    t = np.frombuffer(K.tree_t(), dtype=np.uint8).reshape(1, -1)
    out, st = ctx.rsa_partial_sign(t, [t.shape[1]], be_rows([k["n"]], 256), exps, [f[2] for f in fr], exp_used=[len(f[3]) for f in fr])
    assert (st == R.OK).all() and len(fr) == 40 and exp_len == 2047
    return {(f[0], f[1]): int.from_bytes(out[i].tobytes(), "big") for i, f in enumerate(fr)}


def test_the_device_closes_the_loop_on_the_tree(gpu_ctx):
    k = K.kat()
    digest = hashlib.sha256(k["tbs"]).digest()
    psig = _tree_call(gpu_ctx)
    for (srv, kid), ci in psig.items():                              # byte for byte against the restatement, every one of the forty
        sb, mag = R.stored(K.tree()[srv][kid])
        assert (R.OK, ci) == R.sign(K.tree_t(), k["n"], [(sb, int.from_bytes(mag, "big"))])[0], (srv, kid)
    sigs = []
    for live in K.LIVE_SETS:
        factors = R.client_factors(K.TREE_N, K.TREE_K, live, lambda srv, kid: psig.get((srv, kid)))
        assert factors is not None and len(factors) == (4 if len(live) == 4 else 10)
        s = gpu_ctx.modmul_product([factors], [k["n"]], [0])[0]
        assert s == k["sig"], live
        sigs.append(s.to_bytes(256, "big"))
    valid, st = gpu_ctx.rsa_verify([digest] * len(sigs), sigs, [(k["n"], k["e"])], 8)
    assert (valid == 1).all() and (st == 0).all()
    assert R.client_factors(K.TREE_N, K.TREE_K, (1,), lambda srv, kid: psig.get((srv, kid))) is None
    # one flipped exponent byte in server 0's fragment of the root: the live sets that use it fold to something the verifier refuses
    fr = K.tree_fragments()
    hit = next(i for i, f in enumerate(fr) if f[0] == 0 and f[1] == 0)
    bad = _tree_call(gpu_ctx, flip=hit)
    assert [key for key in psig if psig[key] != bad[key]] == [(0, 0)]
    factors = R.client_factors(K.TREE_N, K.TREE_K, (0, 1), lambda srv, kid: bad.get((srv, kid)))
    s = gpu_ctx.modmul_product([factors], [k["n"]], [0])[0]
    valid, st = gpu_ctx.rsa_verify([digest], [s.to_bytes(256, "big")], [(k["n"], k["e"])], 8)
    assert s != k["sig"] and valid[0] == 0 and st[0] == 0


# ---- 3. widths --------------------------------------------------------------------------------------------------------------------------------
def _width_frags(rng, widths):
    out = []
    for j, w in enumerate(widths):
        mag = rng.getrandbits(8 * w) | (1 << (8 * w - 1))            # exactly w bytes
        out.append((0, K.SIGN_BYTES[j % 4], mag, w))
    return out


def test_row_width_does_not_matter(gpu_ctx):
    """the same fragments in rows of 520 bytes with exp_used, in rows of 520 without it, and in rows of their exact widths"""
    reqs = [(K.kat()["n"], K.tree_t())]
    frags = _width_frags(random.Random(11), [1, 2, 3, 64, 513, 513, 64, 3, 2, 1, 7])
    wide, st = sign_call(gpu_ctx, reqs, frags, 256, 520)
    assert_rows(wide, st, want_rows(reqs, frags, 256))
    padded, st2 = sign_call(gpu_ctx, reqs, frags, 256, 520, used=False)
    assert (padded == wide).all() and (st2 == st).all()
    for w in sorted({f[3] for f in frags}):
        idx = [i for i, f in enumerate(frags) if f[3] == w]
        exact, st3 = sign_call(gpu_ctx, reqs, [frags[i] for i in idx], 256, w, used=False)
        assert (exact == wide[idx]).all() and (st3 == 0).all(), w


@pytest.fixture(scope="module")
def caller_order_ctx(gpu_ctx):
    """a context whose chains run as submitted (BFTKV_PSIGN_ORDER=caller), not longest first: no answer may depend on the order"""
    from bftkv_amd import Context
    os.environ["BFTKV_PSIGN_ORDER"] = "caller"
    try:
        ctx = Context(0)
    finally:
        del os.environ["BFTKV_PSIGN_ORDER"]
    yield ctx
    ctx.close()


def test_sixteen_widths_in_one_wave(gpu_ctx, caller_order_ctx):
    """chains of 1, 2, 3, 64 and 513 used bytes share ONE wave, shuffled: each equals its answer alone -- with the host's order (longest
    first) and as submitted, where the wave's first chain is not its widest"""
    reqs = [(K.kat()["n"], K.tree_t()), (K.moduli()["odd2041"], b"\x33" * 20)]
    rng = random.Random(16)
    frags = _width_frags(rng, [1, 2, 3, 64, 513, 1, 2, 3, 64, 513, 1, 2, 3, 64, 1, 2])
    frags = [(j % 2,) + f[1:] for j, f in enumerate(frags)]
    rng.shuffle(frags)
    assert len(frags) == 16 and frags[0][3] != 513
    alone = [sign_call(gpu_ctx, reqs, [f], 256, f[3], used=False) for f in frags]
    want = want_rows(reqs, frags, 256)
    for j, (o, s) in enumerate(alone):
        assert (int(s[0]), o[0].tobytes()) == want[j], j
    for ctx in (gpu_ctx, caller_order_ctx):
        out, st = sign_call(ctx, reqs, frags, 256, 513)
        assert_rows(out, st, want, "sorted" if ctx is gpu_ctx else "as submitted")
    # the corpus' widest shape as submitted: every class of magnitude at every exp_used, in whatever wave it lands in
    ci = next(i for i, c in enumerate(K.calls()) if c.name == "e513_n128")
    a = K.call_arrays(K.calls()[ci])
    out, st = caller_order_ctx.rsa_partial_sign(a["t"], a["t_len"], a["mods"], a["exps"], a["sign"], a["mod_idx"], a["frag_req"], a["exp_used"])
    assert_rows(out, st, [(s, v.to_bytes(128, "big")) for s, v in K.expected(ci)], "e513_n128 as submitted")


def test_a_wave_of_empty_magnitudes(gpu_ctx):
    """every chain of the call's one wave has exp_used 0, under sign bytes of both kinds: no window at all, from the table straight to
    the leave -- m^0 = 1 in every row"""
    reqs = [(K.kat()["n"], K.tree_t())]
    frags = [(0, 1, 0, 0), (0, 0, 0, 0), (0, 0xFF, 0, 0)]
    out, st = sign_call(gpu_ctx, reqs, frags, 256, 2)
    want = want_rows(reqs, frags, 256)
    assert want == [(R.OK, (1).to_bytes(256, "big"))] * 3
    assert_rows(out, st, want)


def test_more_chains_than_one_launch_takes(gpu_ctx):
    n = TPA_LAUNCH_CHAINS + 17
    mod = K.moduli()["odd520"]
    rng = np.random.default_rng(65)
    exps = rng.integers(0, 256, size=(n, 2), dtype=np.uint8)
    sg = rng.integers(0, 3, size=n, dtype=np.uint8)
    ts = [b"", b"\x5a", K.tree_t()]                                 # (T of the corpus: units under this modulus)
    fr = (np.arange(n) % 3).astype(np.uint32)
    t = np.zeros((3, 51), dtype=np.uint8)
    for i, tt in enumerate(ts):
        t[i, :len(tt)] = np.frombuffer(tt, dtype=np.uint8)
    out, st = gpu_ctx.rsa_partial_sign(t, [len(x) for x in ts], be_rows([mod], 128), exps, sg, frag_req=fr)
    assert (st == R.OK).all()
    ms = [R.emsa_encode(x, mod) for x in ts]
    inv = [pow(m, -1, mod) for m in ms]
    got = [int.from_bytes(out[i].tobytes(), "big") for i in range(n)]
    for i in range(n):
        e = int(exps[i, 0]) << 8 | int(exps[i, 1])
        assert got[i] == pow(inv[i % 3] if sg[i] and e else ms[i % 3], e, mod), i


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------------------
def _raw(lib, h, n_reqs=2, t_cap=51, t_len=(51, 3), n_mods=1, nb=256, n_frags=3, el=8, used=(8, 2, 0), even=False, dirty_front=None, null=()):
    """a direct call with dirty result arrays -> (rc, status, out)"""
    k = K.kat()
    width = min(max(nb, 1), 300)
    d = dict(t=np.full((max(n_reqs, 1), max(t_cap, 1)), 0x21, dtype=np.uint8), tl=np.array(list(t_len) + [0] * 8, dtype=np.uint32),
             mods=be_rows([k["n"] - 1 if even else k["n"]], 256) if width == 256 else be_rows([(1 << (8 * width)) - 1 - (1 if even else 0)], width),
             exps=np.zeros((max(n_frags, 1), max(el, 1)), dtype=np.uint8), used=np.array(list(used) + [0] * 8, dtype=np.uint32),
             sign=np.array([1, 0, 2] * 4, dtype=np.uint8), fr=np.array([0, 1, 1] * 4, dtype=np.uint32),
             out=np.full((max(n_frags, 1), width), 0xA5, dtype=np.uint8), st=np.zeros(max(n_frags, 1), dtype=np.uint8))
    for f in range(min(n_frags, 3)):
        u = min(int(d["used"][f]), max(el, 1))
        d["exps"][f, max(el, 1) - u:] = 0x5A
    if dirty_front is not None:
        d["exps"][dirty_front, 0] = 1
    g8 = lambda key: None if key in null else P8(d[key])             # noqa: E731
    g32 = lambda key: None if key in null else A32(d[key])           # noqa: E731
    rc = lib.bftkv_gpu_rsa_partial_sign(h, n_reqs, g8("t"), t_cap, g32("tl"), None, n_mods, g8("mods"), nb, n_frags, g32("fr"), g8("exps"), el, g32("used"),
                                        g8("sign"), g8("out"), g8("st"))
    return rc, d["st"], d["out"]


REFUSALS = [dict(nb=0), dict(nb=257), dict(el=0), dict(el=8201), dict(t_cap=257), dict(nb=128, t_cap=129), dict(t_len=(52, 3)), dict(t_len=(51, 52)),
            dict(used=(9, 2, 0)), dict(used=(8, 2, 9)), dict(dirty_front=1), dict(dirty_front=2), dict(n_reqs=0), dict(n_frags=0), dict(n_mods=0),
            dict(null=("t",)), dict(null=("tl",)), dict(null=("mods",)), dict(null=("exps",)), dict(null=("sign",))]


def test_refusals_of_the_direct_entry(gpu_ctx):
    lib, h = gpu_ctx.lib, gpu_ctx.h
    good = _raw(lib, h)
    assert good[0] == 0 and [int(s) for s in good[1]] == [0, 0, 0] and good[2][:2].any(axis=1).all() and int.from_bytes(good[2][2].tobytes(), "big") == 1
    for kw in REFUSALS:
        rc, st, out = _raw(lib, h, **kw)
        assert rc == E_INVALID, (kw, rc)
        if kw.get("n_frags", 3):
            assert (st == R.FAILED).all() and not out.reshape(-1)[:3 * kw.get("nb", 256)].any(), kw
    for kw in (dict(null=("out",)), dict(null=("st",))):
        rc, st, out = _raw(lib, h, **kw)
        assert rc == E_INVALID and ("st" in kw["null"] or (st == R.FAILED).all()) and ("out" in kw["null"] or not out.any()), kw
    rc, st, out = _raw(lib, h, even=True)
    assert rc == E_UNSUPPORTED and (st == R.FAILED).all() and not out.any()
    rc, st, out = _raw(lib, None)
    assert rc == E_INVALID and (st == R.FAILED).all() and not out.any()
    for kw in (dict(el=8200, used=(8, 2, 0)), dict(null=("used",), el=2), dict(null=("fr",)), dict(t_cap=0, t_len=(0, 0), null=("t",))):      # no refusals
        rc, st, out = _raw(lib, h, **kw)
        assert rc == 0 and (st == R.OK).all(), kw
    again = _raw(lib, h)                                              # the next good call is unaffected
    assert again[0] == 0 and (again[1] == good[1]).all() and (again[2] == good[2]).all()


# ---- 5. the batcher ----------------------------------------------------------------------------------------------------------------------------
def test_32_threads_through_the_batcher(gpu_ctx):
    """two shapes, fragment counts 1 to 9; among the callers one refused (a byte ahead of exp_used), one even modulus and one request whose m
    has no inverse: everybody gets the direct entry's bytes, and nobody's answer moves"""
    from bftkv_amd import Batcher
    k = K.kat()
    n3, t_bad, _ = K.no_inverse_case()
    rng = random.Random(32)
    mods = [k["n"], K.moduli()["odd2041"], K.moduli()["odd1024"], n3]
    ts = [K.tree_t(), b"", b"\xff" * 40, K.digest_infos()[10]]
    callers = []
    for j in range(32):
        el = (5, 64)[j % 2]
        n_frags = 1 + j % 9
        frags = [(K.SIGN_BYTES[rng.randrange(4)], rng.getrandbits(8 * rng.randrange(1, el + 1)) if rng.randrange(6) else 0) for _ in range(n_frags)]
        callers.append(dict(n=mods[j % 3], t=ts[(j // 3) % 4], el=el, frags=frags, used=[max((m.bit_length() + 7) // 8, rng.randrange(0, el + 1)) for _, m in frags]))
    callers[7].update(n=n3, t=t_bad, frags=[(1, 77), (0, 77), (2, 0), (0xFF, 1 << 30)], used=[5, 5, 0, 5], el=5)      # no inverse
    callers[12]["n"] = k["n"] - 1                                     # an even modulus
    callers[21].update(frags=[(0, 0x0101)] * 2, used=[1, 2])          # refused: a non-zero byte ahead of its exp_used
    direct = {}
    for j, c in enumerate(callers):
        if j in (12, 21):
            continue
        reqs = [(c["n"], c["t"])]
        fr = [(0, sb, mag, u) for (sb, mag), u in zip(c["frags"], c["used"])]
        out, st = sign_call(gpu_ctx, reqs, fr, 256, c["el"])
        assert_rows(out, st, want_rows(reqs, fr, 256), j)
        direct[j] = ([int(s) for s in st], out.tobytes())
    assert direct[7][0] == [R.NO_INVERSE, 0, 0, R.NO_INVERSE]
    b = Batcher(gpu_ctx, max_items=32, max_wait_us=5000, n_lanes=2)
    got = [None] * 32
    gate = threading.Barrier(32)

    def run(j):
        c = callers[j]
        exps = be_rows([m for _, m in c["frags"]], c["el"])
        gate.wait()
        got[j] = b.rsa_partial_sign(c["t"], c["n"].to_bytes(256, "big"), exps, [sb for sb, _ in c["frags"]], exp_used=c["used"])

    th = [threading.Thread(target=run, args=(j,)) for j in range(32)]
    for t_ in th:
        t_.start()
    for t_ in th:
        t_.join()
    stats = b.stats()
    for j in range(32):
        rc, st, out = got[j]
        if j in (12, 21):
            assert rc == (E_UNSUPPORTED if j == 12 else E_INVALID) and (st == R.FAILED).all() and not out.any(), j
        else:
            assert (rc, [int(s) for s in st], out.tobytes()) == (0,) + direct[j], j
    assert stats["calls"] == 30 and stats["batches"] < 30 and stats["max_batch"] > 1, stats
    # what the direct entry refuses for the whole call refuses a lone caller too, before it joins a batch
    one = np.array([[0, 0, 0, 0, 9]], dtype=np.uint8)
    mod = k["n"].to_bytes(256, "big")
    for kw in (dict(t=b"x" * 257), dict(mod=b"\x01" * 257), dict(exps=np.zeros((1, 8201), dtype=np.uint8)), dict(exp_used=[6]), dict(exp_used=[0]), dict(sign=[])):
        a = dict(dict(t=b"abc", mod=mod, exps=one, sign=[1], exp_used=[1]), **kw)
        rc, st, out = b.rsa_partial_sign(a["t"], a["mod"], a["exps"], a["sign"], exp_used=a["exp_used"])
        assert rc == E_INVALID and (st == R.FAILED).all() and not out.any(), list(kw)
    rc, st, out = b.rsa_partial_sign(b"abc", b"\0" * 256, one, [1], exp_used=[1])      # N = 0: a refused request, not an even modulus
    assert rc == 0 and [int(s) for s in st] == [R.INVALID_INPUT] and not out.any()
    rc, st, out = b.rsa_partial_sign(b"abc", mod, one, [1], exp_used=[1])
    assert (rc, int(st[0]), out[0].tobytes()) == (0,) + want_rows([(k["n"], b"abc")], [(0, 1, 9, 1)], 256)[0]
    b.close()
