"""-m gpu: verification of raw DSA signatures (crypto/dsa.Verify, Go 1.13) on the device, groups and keys sent with the call, byte
for byte (valid, status) against the restatement with its rules (tests/dsa_verify_ref.py)."""
import ctypes as C
import functools
import json
import os
import threading

import numpy as np
import pytest

import dsa_verify_cases as K
import dsa_verify_ref as V

pytestmark = pytest.mark.gpu
E_INVALID, E_UNSUPPORTED = -1, -4
FAILED = 0xFF
GPU_NAMES = [g.name for g in K.groups() if g.pbytes <= 256]          # (the 3072-bit group is refused: test_return_codes)


def _want(cases):
    return [V.verify(cs.p, cs.q, cs.g, cs.y, cs.digest, cs.r, cs.s) for cs in cases]


def _call(ctx, G, cases):
    gs, ks, idx = K.tables(cases)
    valid, st = ctx.dsa_verify([cs.digest for cs in cases], [K.sig_bytes(G, cs.r, cs.s) for cs in cases], ks, gs, key_idx=idx, pbytes=G.pbytes,
                               qbytes=G.qbytes)
    return [(int(v), int(s)) for v, s in zip(valid, st)]


def _run(ctx, G, cases):
    """One device call per digest length (a call has one dlen), every case under its own group and key rows."""
    got = [None] * len(cases)
    for _, idx in K.by_dlen(cases).items():
        for i, g in zip(idx, _call(ctx, G, [cases[i] for i in idx])):
            got[i] = g
    return got


@pytest.fixture(scope="module", params=[4, 8])
def lane_ctx(request):
    """A context made while BFTKV_MULTIEXP_LANES names one lane form (the variable is read when a context is created)."""
    import torch  # noqa: F401
    from bftkv_amd import Context
    old = os.environ.get("BFTKV_MULTIEXP_LANES")
    os.environ["BFTKV_MULTIEXP_LANES"] = str(request.param)
    try:
        ctx = Context(0)
    finally:
        if old is None:
            del os.environ["BFTKV_MULTIEXP_LANES"]
        else:
            os.environ["BFTKV_MULTIEXP_LANES"] = old
    yield ctx
    ctx.close()


def _check_corpus(ctx, name):
    G = K.group(name)
    cases = K.corpus(name)
    want, got = _want(cases), _run(ctx, G, cases)
    for cs, w, g in zip(cases, want, got):
        print(name, cs.label, "want", w, "got", g)
    bad = [(cs.label, w, g) for cs, w, g in zip(cases, want, got) if w != g]
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", GPU_NAMES)
def test_corpus(gpu_ctx, name):
    _check_corpus(gpu_ctx, name)


def test_corpus_under_each_lane_form(lane_ctx):
    for name in GPU_NAMES:
        _check_corpus(lane_ctx, name)


def _cycle(name, n):
    """n cases of one digest length out of a group's corpus, repeated as often as it takes."""
    G = K.group(name)
    pool = [cs for cs in K.corpus(name) if len(cs.digest) == G.q.bit_length() // 8]
    return G, [pool[i % len(pool)] for i in range(n)]


@pytest.mark.parametrize("n_ops", [1, 2, 33, 63, 64, 65])
def test_sizes_at_the_block_edges(lane_ctx, n_ops):
    """64 lane groups make a block at 4 lanes, 32 at 8: one under, exactly, one over, and a lone signature."""
    for name in ("p2047_q224", "p1025_q256"):
        G, cases = _cycle(name, n_ops)
        assert _call(lane_ctx, G, cases) == _want(cases), (name, n_ops)


def test_more_keys_than_signatures(gpu_ctx):
    G, cases = _cycle("p1023_q224", 3)
    cs = cases[0]
    assert _want([cs]) == [(1, V.OK)]
    gs = [(cs.p, cs.q, cs.g)]
    # n_ops = 1, n_keys = 5: the fourth key is the signer's
    ks = [(0, (cs.y * 3 + j) % cs.p) for j in range(3)] + [(0, cs.y), (0, 1)]
    for ki, expect in ((3, 1), (0, 0), (4, 0)):
        valid, st = gpu_ctx.dsa_verify([cs.digest], [K.sig_bytes(G, cs.r, cs.s)], ks, gs, key_idx=[ki], pbytes=G.pbytes, qbytes=G.qbytes)
        assert (int(valid[0]), int(st[0])) == (expect, V.OK) == V.verify(cs.p, cs.q, cs.g, ks[ki][1], cs.digest, cs.r, cs.s)
    # 3 signatures, 9 keys (most of them nobody's)
    ks = [(0, (cs.y + 7 * j) % cs.p) for j in range(1, 9)] + [(0, cs.y)]
    idx = [8, 2, 8]
    valid, st = gpu_ctx.dsa_verify([c.digest for c in cases], [K.sig_bytes(G, c.r, c.s) for c in cases], ks, gs, key_idx=idx, pbytes=G.pbytes, qbytes=G.qbytes)
    want = [V.verify(c.p, c.q, c.g, ks[i][1], c.digest, c.r, c.s) for c, i in zip(cases, idx)]
    assert [(int(v), int(s)) for v, s in zip(valid, st)] == want and want[1] == (0, V.OK)


def _standard(name, i=0):
    k = json.load(open(os.path.join(K.GOLDEN, "keys_%s.json" % name)))["keys"][i]
    p, q, g, x = (int(k[f], 16) for f in ("p", "q", "g", "x"))
    return p, q, g, x, pow(g, x, p)


def _sign(rng, p, q, g, x, dg):
    rs = None
    while rs is None:
        rs = K.sign(p, q, g, x, dg, K.rnd(rng, q) or 1)
    return rs


def test_mixed_groups_in_one_call(gpu_ctx):
    """pbytes = 256 and qbytes = 32 over the 1024/160, 1536/224 and 2048/256 groups: at dlen = 20 every signature is answered, at
    dlen = 32 exactly those under the shorter orders are fenced."""
    rng = np.random.default_rng(4)
    grp = [_standard(n) for n in ("dsa1024", "dsa1536", "dsa2048")]
    gs, ks = [(p, q, g) for p, q, g, _, _ in grp], [(i, t[4]) for i, t in enumerate(grp)]
    sig = lambda r, s: r.to_bytes(32, "big") + s.to_bytes(32, "big")        # noqa: E731
    for dlen in (20, 32):
        digests, sigs, idx, want = [], [], [], []
        for j in range(18):
            gi = j % 3
            p, q, g, x, y = grp[gi]
            dg = rng.bytes(dlen)
            # (signed over what fits the order, so that the signature is honest wherever it is answered)
            r, s = _sign(rng, p, q, g, x, dg if dlen <= q.bit_length() // 8 else dg[:q.bit_length() // 8])
            if j % 6 >= 3:
                s = s ^ 1
            digests.append(dg); sigs.append(sig(r, s)); idx.append(gi)
            want.append(V.verify(p, q, g, y, dg, r, s))
        valid, st = gpu_ctx.dsa_verify(digests, sigs, ks, gs, key_idx=idx, pbytes=256, qbytes=32)
        got = [(int(v), int(s)) for v, s in zip(valid, st)]
        assert got == want, dlen
        if dlen == 20:
            assert all(s == V.OK for _, s in got) and [v for v, _ in got] == [1, 1, 1, 0, 0, 0] * 3
        else:
            assert [s for _, s in got] == [V.FENCED, V.FENCED, V.OK] * 6
            assert [v for v, _ in got][2::3] == [1, 0] * 3
            # the answered ones are what they are in a call of their own
            mine = [j for j in range(18) if idx[j] == 2]
            v2, s2 = gpu_ctx.dsa_verify([digests[j] for j in mine], [sigs[j] for j in mine], [(0, grp[2][4])], [gs[2]], pbytes=256, qbytes=32)
            assert [(int(a), int(b)) for a, b in zip(v2, s2)] == [got[j] for j in mine]


@functools.lru_cache(maxsize=None)
def _volume(n_keys):
    """2,000 honest signatures under n_keys keys of keys_dsa2048.json (each key in its own group), every 7th one mutated."""
    rng = np.random.default_rng(2000 + n_keys)
    grp = [_standard("dsa2048", i) for i in range(n_keys)]
    digests, sigs, idx, expect = [], [], [], []
    for i in range(2000):
        ki = int(rng.integers(n_keys))
        p, q, g, x, _ = grp[ki]
        dg = rng.bytes(32)
        r, s = _sign(rng, p, q, g, x, dg)
        ok = 1
        if i % 7 == 3:
            ok = 0
            which = (i // 7) % 4
            if which == 0:
                r ^= 1 << int(rng.integers(256))
            elif which == 1:
                s ^= 1 << int(rng.integers(256))
            elif which == 2:
                dg = bytes(K.flip_int(int.from_bytes(dg, "big"), int(rng.integers(256))).to_bytes(32, "big"))
            elif n_keys > 1:
                ki = (ki + 1) % n_keys
            else:
                r, s = s, r
        digests.append(dg); sigs.append(r.to_bytes(32, "big") + s.to_bytes(32, "big")); idx.append(ki); expect.append(ok)
    return grp, digests, sigs, idx, np.array(expect, dtype=np.uint8)


@pytest.mark.parametrize("n_keys", [1, 100])
def test_two_thousand(gpu_ctx, n_keys):
    grp, digests, sigs, idx, expect = _volume(n_keys)
    gs, ks = [(p, q, g) for p, q, g, _, _ in grp], [(i, t[4]) for i, t in enumerate(grp)]
    valid, st = gpu_ctx.dsa_verify(digests, sigs, ks, gs, key_idx=None if n_keys == 1 else idx, pbytes=256, qbytes=32)
    assert not st.any(), np.flatnonzero(st)[:8]                          # nothing fenced, nothing failed
    assert (valid == expect).all(), np.flatnonzero(valid != expect)[:8]
    assert expect.sum() == 2000 - len(range(3, 2000, 7))
    rng = np.random.default_rng(16)
    for i in [int(v) for v in rng.choice(2000, 12, replace=False)] + [3, 10, 17, 24]:
        p, q, g, _, y = grp[idx[i]]
        r, s = int.from_bytes(sigs[i][:32], "big"), int.from_bytes(sigs[i][32:], "big")
        assert (int(valid[i]), int(st[i])) == V.verify(p, q, g, y, digests[i], r, s), i


def _raw(cases, G):
    gs, ks, idx = K.tables(cases)
    from bftkv_amd._native import _ints_to_be
    a = lambda b: np.frombuffer(b, dtype=np.uint8).copy()          # noqa: E731
    return dict(n=len(cases), dg=a(b"".join(cs.digest for cs in cases)), dlen=len(cases[0].digest),
                sg=a(b"".join(K.sig_bytes(G, cs.r, cs.s) for cs in cases)), idx=np.array(idx, dtype=np.uint32), n_keys=len(ks),
                y=_ints_to_be([k[1] for k in ks], G.pbytes), kg=np.array([k[0] for k in ks], dtype=np.uint32), n_groups=len(gs),
                p=_ints_to_be([g[0] for g in gs], G.pbytes), q=_ints_to_be([g[1] for g in gs], G.qbytes), g=_ints_to_be([g[2] for g in gs], G.pbytes))


P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)        # noqa: E731


def test_key_and_group_indices_are_clamped_and_null_means_zero(gpu_ctx):
    rng = np.random.default_rng(9)
    grp = [_standard("dsa2048", i) for i in range(2)]
    gs = [(p, q, g) for p, q, g, _, _ in grp]
    ks = [(0, grp[0][4]), (7, grp[1][4]), (0xFFFFFFFF, grp[1][4])]                  # groups 7 and 2^32 - 1 are group 1
    eff = [0, 1, 1]
    digests = [rng.bytes(32) for _ in range(6)]
    signer = [0, 1, 2, 1, 2, 0]
    sigs = []
    for dg, k in zip(digests, signer):
        p, q, g, x, _ = grp[eff[k]]
        r, s = _sign(rng, p, q, g, x, dg)
        sigs.append(r.to_bytes(32, "big") + s.to_bytes(32, "big"))
    key_idx = [0, 1, 2, 9, 0xFFFFFFFF, 1]                                          # keys 9 and 2^32 - 1 are key 2
    used = [0, 1, 2, 2, 2, 1]
    want = [V.verify(*gs[eff[u]], ks[u][1], dg, int.from_bytes(sg[:32], "big"), int.from_bytes(sg[32:], "big")) for u, dg, sg in zip(used, digests, sigs)]
    assert [v for v, _ in want] == [1, 1, 1, 1, 1, 0]
    valid, st = gpu_ctx.dsa_verify(digests, sigs, ks, gs, key_idx=key_idx, pbytes=256, qbytes=32)
    assert [(int(v), int(s)) for v, s in zip(valid, st)] == want
    # NULL key_idx: key 0 for all
    valid, st = gpu_ctx.dsa_verify(digests, sigs, ks, gs, pbytes=256, qbytes=32)
    assert [int(v) for v in valid] == [1, 0, 0, 0, 0, 1] and not st.any()
    # NULL key_group: every key in group 0 (the raw entry; the binding always sends the array)
    from bftkv_amd._native import _ints_to_be
    lib, h = gpu_ctx.lib, gpu_ctx.h
    a = lambda b: np.frombuffer(b, dtype=np.uint8).copy()          # noqa: E731
    dg, sg, ki = a(b"".join(digests)), a(b"".join(sigs)), np.array([0, 1, 1, 1, 1, 0], dtype=np.uint32)
    y = _ints_to_be([grp[0][4], grp[1][4]], 256)
    p, q, g = (_ints_to_be([t[i] for t in gs], w) for i, w in ((0, 256), (1, 32), (2, 256)))
    valid, st = np.full(6, 0xAA, dtype=np.uint8), np.full(6, 0xAA, dtype=np.uint8)
    assert lib.bftkv_gpu_dsa_verify(h, 6, P(dg), 32, P(sg), 32, P(ki), 2, P(y), None, 256, 2, P(p), P(q), P(g), P(valid), P(st)) == 0
    want = [V.verify(*gs[0], [grp[0][4], grp[1][4]][k], d, int.from_bytes(s_[:32], "big"), int.from_bytes(s_[32:], "big")) for k, d, s_ in zip(ki, digests, sigs)]
    assert [(int(v), int(s)) for v, s in zip(valid, st)] == want and [v for v, _ in want] == [1, 0, 0, 0, 0, 1]


def test_device_form_against_host_form(gpu_ctx):
    import torch
    lib, h = gpu_ctx.lib, gpu_ctx.h
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")    # noqa: E731
    for name in ("composite_q160", "p2048_q256", "p512_q8"):
        G, _ = _cycle(name, 1)
        dlen = max(K.by_dlen(K.corpus(name)))                                # (the fenced ones: one byte more than the order)
        for cases in ([cs for cs in K.corpus(name) if len(cs.digest) == dlen], _cycle(name, 70)[1]):
            a = _raw(cases, G)
            n = a["n"]
            want = _want(cases)
            valid, st = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
            args = (a["n_keys"], P(a["y"]), P(a["kg"]), G.pbytes, a["n_groups"], P(a["p"]), P(a["q"]), P(a["g"]))
            gpu_ctx._check(lib.bftkv_gpu_dsa_verify(h, n, P(a["dg"]), a["dlen"], P(a["sg"]), G.qbytes, P(a["idx"]), *args, P(valid), P(st)), "dsa_verify")
            assert [(int(v), int(s)) for v, s in zip(valid, st)] == want
            d_dg, d_sg, d_ki = up(a["dg"]), up(a["sg"]), up(a["idx"].view(np.int32))
            d_valid = torch.full((n + 8,), 0x55, dtype=torch.uint8, device="cuda:0")
            d_st = torch.full((n + 8,), 0x55, dtype=torch.uint8, device="cuda:0")
            gpu_ctx._check(lib.bftkv_gpu_dsa_verify_dev(h, n, d_dg.data_ptr(), a["dlen"], d_sg.data_ptr(), G.qbytes, d_ki.data_ptr(), *args,
                                                        d_valid.data_ptr(), d_st.data_ptr()), "dsa_verify_dev")
            gpu_ctx.sync()
            assert (d_valid.cpu().numpy()[:n] == valid).all() and (d_st.cpu().numpy()[:n] == st).all(), name
            assert (d_valid.cpu().numpy()[n:] == 0x55).all() and (d_st.cpu().numpy()[n:] == 0x55).all()      # nothing past n_ops


def test_return_codes(gpu_ctx):
    lib, h = gpu_ctx.lib, gpu_ctx.h
    G, cases = _cycle("p1023_q224", 4)
    a = _raw(cases, G)
    n = a["n"]

    def call(n_ops=n, dg=a["dg"], dlen=a["dlen"], sg=a["sg"], qb=G.qbytes, idx=a["idx"], n_keys=a["n_keys"], y=a["y"], kg=a["kg"], pb=G.pbytes,
             n_groups=a["n_groups"], p=a["p"], q=a["q"], g=a["g"], out=True, ctx=h):
        valid, st = np.full(n + 4, 0xAA, dtype=np.uint8), np.full(n + 4, 0xAA, dtype=np.uint8)
        rc = lib.bftkv_gpu_dsa_verify(ctx, n_ops, P(dg), dlen, P(sg), qb, P(idx), n_keys, P(y), P(kg), pb, n_groups, P(p), P(q), P(g),
                                      P(valid) if out else None, P(st) if out else None)
        return rc, valid, st

    rc, valid, st = call()
    assert rc == 0 and [(int(v), int(s)) for v, s in zip(valid[:n], st[:n])] == _want(cases)
    assert (valid[n:] == 0xAA).all() and (st[n:] == 0xAA).all()
    rc, valid, st = call(n_ops=0)
    assert rc == 0 and (valid == 0xAA).all() and (st == 0xAA).all()
    assert lib.bftkv_gpu_dsa_verify(h, 0, None, 28, None, G.qbytes, None, 1, P(a["y"]), None, G.pbytes, 1, P(a["p"]), P(a["q"]), P(a["g"]), None, None) == 0
    even_p, even_q = a["p"].copy(), a["q"].copy()
    even_p[0, -1] &= 0xFE
    even_q[0, -1] &= 0xFE
    refused = [(dict(p=even_p), E_UNSUPPORTED), (dict(q=even_q), E_UNSUPPORTED), (dict(pb=384), E_INVALID), (dict(pb=0), E_INVALID), (dict(qb=33), E_INVALID),
               (dict(qb=0), E_INVALID), (dict(dlen=0), E_INVALID), (dict(dlen=65), E_INVALID), (dict(n_keys=0), E_INVALID), (dict(n_groups=0), E_INVALID),
               (dict(dg=None), E_INVALID), (dict(sg=None), E_INVALID), (dict(y=None), E_INVALID), (dict(p=None), E_INVALID), (dict(q=None), E_INVALID),
               (dict(g=None), E_INVALID)]
    for kw, code in refused:
        rc, valid, st = call(**kw)
        assert rc == code, (list(kw), rc)
        assert (st[:n] == FAILED).all() and (valid[:n] == 0).all(), list(kw)             # fail closed
        assert (valid[n:] == 0xAA).all() and (st[n:] == 0xAA).all()
    assert call(out=False)[0] == E_INVALID and call(ctx=None)[0] == E_INVALID
    # the 3072-bit group of the key files: its width is out of range
    p, q, g, x, y = _standard("dsa3072")
    with pytest.raises(Exception, match=r"\(-1\)"):
        gpu_ctx.dsa_verify([bytes(32)], [bytes(64)], [(0, y)], [(p, q, g)])
    # the batcher: bad arguments fail closed, an even modulus is this caller's alone
    from bftkv_amd import Batcher
    cs = cases[0]
    assert _want([cs]) == [(1, V.OK)]
    v1, s1 = np.full(1, 0xAA, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
    one = _raw([cs], G)
    bargs = lambda b, p=one["p"], dlen=one["dlen"]: (b, P(one["dg"]), dlen, P(one["sg"]), G.qbytes, P(one["y"]), G.pbytes, P(p), P(one["q"]), P(one["g"]), P(v1), P(s1))    # noqa: E731
    assert lib.bftkv_gpu_batcher_dsa_verify(*bargs(None)) == E_INVALID and (int(v1[0]), int(s1[0])) == (0, FAILED)
    b = Batcher(gpu_ctx, max_items=8, n_lanes=1)
    v1[0], s1[0] = 0xAA, 0
    assert lib.bftkv_gpu_batcher_dsa_verify(*bargs(b.h, dlen=0)) == E_INVALID and (int(v1[0]), int(s1[0])) == (0, FAILED)
    v1[0], s1[0] = 0xAA, 0
    assert lib.bftkv_gpu_batcher_dsa_verify(*bargs(b.h, p=even_p[:1])) == E_UNSUPPORTED and (int(v1[0]), int(s1[0])) == (0, FAILED)
    assert lib.bftkv_gpu_batcher_dsa_verify(*bargs(b.h)) == 0 and (int(v1[0]), int(s1[0])) == (1, V.OK)
    b.close()


def test_batcher_mixed_groups(gpu_ctx):
    """64 threads, one signature per call, three groups and two digest lengths, valid, invalid, fenced and no-inverse mixed; one
    caller brings an even p and is refused alone."""
    from bftkv_amd import Batcher
    jobs = []
    for name in ("composite_q160", "p1023_q224", "dsa2048"):
        G = K.group(name)
        qb = G.q.bit_length() // 8
        jobs += [(G, cs) for cs in K.corpus(name) if len(cs.digest) in (qb, qb + 1)]
    rng = np.random.default_rng(64)
    jobs = [jobs[int(i)] for i in rng.permutation(len(jobs))][:128]
    want = [V.verify(cs.p, cs.q, cs.g, cs.y, cs.digest, cs.r, cs.s) for _, cs in jobs]
    assert {w for w in want} == {(1, V.OK), (0, V.OK), (0, V.FENCED), (0, V.NO_INVERSE)}
    assert len({len(cs.digest) for G, cs in jobs if G.name == "dsa2048"}) == 2
    b = Batcher(gpu_ctx, max_items=64, n_lanes=2)
    got = [None] * len(jobs)
    odd = {}

    def run(lo):
        for i in range(lo, len(jobs), 64):
            G, cs = jobs[i]
            got[i] = b.dsa_verify(cs.digest, K.sig_bytes(G, cs.r, cs.s), (cs.p, cs.q, cs.g), cs.y, pbytes=G.pbytes)
        if lo == 5:
            G, cs = jobs[lo]
            odd["even p"] = b.dsa_verify(cs.digest, K.sig_bytes(G, cs.r, cs.s), (cs.p - 1, cs.q, cs.g), cs.y, pbytes=G.pbytes)

    th = [threading.Thread(target=run, args=(i,)) for i in range(64)]
    for t_ in th:
        t_.start()
    for t_ in th:
        t_.join()
    b.close()
    for i, (w, g) in enumerate(zip(want, got)):
        assert g == (0, w[1], w[0]), (i, jobs[i][0].name, jobs[i][1].label, w, g)
    assert odd["even p"] == (E_UNSUPPORTED, FAILED, 0)
