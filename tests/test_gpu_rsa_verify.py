"""GPU: raw RSA PKCS#1 v1.5 verification (bftkv_gpu_rsa_verify, its _dev form and the batcher kind) against the Python restatement
(tests/rsa_verify_ref.py) over the seeded corpus (tests/rsa_verify_cases.py), byte for byte in (valid, status), on the default
context and under each lane form of k_rsav_verify (<18, 4, 29> and <10, 8>, BFTKV_RSAV_LANES)."""
import ctypes as C
import functools
import hashlib
import json
import os
import threading

import numpy as np
import pytest

import rsa_verify_cases as K
import rsa_verify_ref as V

pytestmark = pytest.mark.gpu

E_INVALID, FAILED = -1, 0xFF
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)        # noqa: E731
CELL_IDS = ["hash%d_dlen%d" % c for c in K.HASH_CELLS]


@pytest.fixture(scope="module", params=[4, 8], ids=["lanes4", "lanes8"])
def rsav_ctx(request):
    """A context made while BFTKV_RSAV_LANES names one lane form (the variable is read when a context is created)."""
    import torch  # noqa: F401
    from bftkv_amd import Context
    old = os.environ.get("BFTKV_RSAV_LANES")
    os.environ["BFTKV_RSAV_LANES"] = str(request.param)
    try:
        ctx = Context(0)
    finally:
        if old is None:
            del os.environ["BFTKV_RSAV_LANES"]
        else:
            os.environ["BFTKV_RSAV_LANES"] = old
    yield ctx
    ctx.close()


def call(ctx, cases, nbytes=256):
    dg, sg, keys, idx = K.call_arrays(cases, nbytes)
    valid, st = ctx.rsa_verify(dg, sg, keys, cases[0].hash_id, key_idx=idx, nbytes=nbytes)
    return [(int(v), int(s)) for v, s in zip(valid, st)]


def want(cases):
    return [V.verify(c.n, c.e, c.hash_id, c.digest, c.s) for c in cases]


def check(ctx, cases, nbytes=256):
    got, exp = call(ctx, cases, nbytes), want(cases)
    bad = [(c.key, c.label, g, w) for c, g, w in zip(cases, got, exp) if g != w]
    assert not bad, (len(bad), bad[:6])


def fitting(cases, nbytes=256):
    return [c for c in cases if c.min_nbytes <= nbytes]


@pytest.mark.parametrize("cellid", K.HASH_CELLS, ids=CELL_IDS)
def test_corpus_on_the_default_context(gpu_ctx, cellid):
    cases = fitting(K.corpus(*cellid))
    assert len(cases) > 400            # (SHA-512 fits the fewest keys: 435 cases)
    check(gpu_ctx, cases)


def test_corpus_under_each_lane_form(rsav_ctx):
    for cellid in K.HASH_CELLS:
        check(rsav_ctx, fitting(K.corpus(*cellid)))


@functools.lru_cache(maxsize=None)
def _pool():
    """Cases of SHA-256 with a verdict either way, from keys of every size class that carries the hash."""
    cases = [c for c in fitting(K.corpus(8, 32)) if c.part in ("honest", "mutation", "forgery", "wide", "exponent", "key")]
    rng = np.random.default_rng(8)
    return [cases[int(i)] for i in rng.permutation(len(cases))]


@pytest.mark.parametrize("n_ops", [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129])
def test_sizes_at_the_group_wave_and_block_edges(rsav_ctx, n_ops):
    """16 signatures make a wave and 64 a block at 4 lanes, 8 and 32 at 8 lanes: one under, exactly, one over, and a lone signature."""
    pool = _pool()
    cases = [pool[(n_ops + i) % len(pool)] for i in range(n_ops)]
    check(rsav_ctx, cases)


def _class_cases(n_sigs):
    """Signatures whose keys cycle through the exponent classes: popcount 1 (65536), 2 (3 or 65537), more (7.., 65539.., 2^32 - 1..),
    even (2), 0 and 1, each with the x-shortcut on (s < 2^(8k)) and off (the same residue carried at or above 2^(8k))."""
    by_e = {}
    for name in ("rsa1024", "rsa1016", "rsa1025e3"):
        k = K.key(name)
        for c in K.exponent_cases(name) + tuple(c for c in K.cell(name, 8, 32) if c.part in ("honest", "mutation")):
            wide = c.s % c.n + (c.n << (8 * k.k - c.n.bit_length() + 3))
            by_e.setdefault((c.e, False), []).append(c)
            by_e.setdefault((c.e, True), []).append(K.Case(c.label + ", carried above 2^(8k)", c.part, c.key, c.n, c.e, c.hash_id, c.digest, wide))
    es = sorted({e for e, _ in by_e}, key=lambda e: (bin(e).count("1") % 3, e))          # neighbours differ in their popcount class
    out = []
    for i in range(n_sigs):
        lst = by_e[(es[i % len(es)], (i // len(es)) % 2 == 1)]
        out.append(lst[(i // 3) % len(lst)])
    classes = {(c.e, c.s >> (8 * ((c.n.bit_length() + 7) // 8)) != 0) for c in out}
    pops = {bin(c.e).count("1") for c in out}
    assert len(classes) >= 6 and {0, 1, 2} <= pops and any(p > 2 for p in pops) and any(c.e % 2 == 0 and c.e for c in out)
    assert any(w for _, w in classes) and any(not w for _, w in classes) and len({v for v, _ in want(out)}) == 2
    return out


@pytest.mark.parametrize("n_sigs", [16, 64])
def test_exponent_classes_within_one_wave_and_one_block(rsav_ctx, n_sigs):
    check(rsav_ctx, _class_cases(n_sigs))


def test_every_modulus_size_in_one_call_then_each_at_its_own_width(rsav_ctx):
    """A short modulus leaves upper lanes of n empty.  Hash id 0 at one digest byte: every key of the corpus carries it."""
    per_key = {k.name: [c for c in K.cell(k.name, 0, 1) if c.part in ("honest", "mutation", "forgery", "value")] for k in K.keys()}
    every = [c for cs in per_key.values() for c in cs]
    assert len({c.n.bit_length() for c in every if c.part == "honest"}) >= 26
    check(rsav_ctx, fitting(every))
    for k in K.keys():
        check(rsav_ctx, fitting(per_key[k.name], k.k), nbytes=k.k)


def test_more_keys_than_signatures_clamped_and_null_indices(gpu_ctx):
    ks = [k for k in K.keys() if k.k >= 62]
    keys = [(k.n, k.e) for k in ks] * 3                                    # ~50 keys, 4 signatures
    hon = [next(c for c in K.cell(k.name, 8, 32) if c.part == "honest") for k in ks]
    pick = [0, len(ks) - 1, 5, len(keys) - 1]
    dg = [hon[i % len(ks)].digest for i in pick]
    sg = [hon[i % len(ks)].s.to_bytes(256, "big") for i in pick]
    valid, st = gpu_ctx.rsa_verify(dg, sg, keys, 8, key_idx=pick, nbytes=256)
    assert valid.tolist() == [1, 1, 1, 1] and not st.any()
    # an index past the table is the last key; NULL is key 0
    valid, st = gpu_ctx.rsa_verify(dg, sg, keys, 8, key_idx=[0, 0xFFFFFFFF, len(keys), len(keys) - 1], nbytes=256)
    assert valid.tolist() == [1, 1, 0, 1] and not st.any()
    valid, st = gpu_ctx.rsa_verify(dg, sg, keys, 8, nbytes=256)
    assert valid.tolist() == [1, 0, 0, 0] and not st.any()
    valid, st = gpu_ctx.rsa_verify([dg[3]] * 2, [sg[3]] * 2, keys, 8, key_idx=[7 * len(keys), 1], nbytes=256)
    assert valid.tolist() == [1, 0] and not st.any()


@functools.lru_cache(maxsize=None)
def _volume(n_keys):
    """2,000 SHA-256 signatures under n_keys RSA-2048 keys, drawn from 200 signed ones, every 7th mutated (signature or digest)."""
    rng = np.random.default_rng(2000 + n_keys)
    raw = json.load(open(os.path.join(K.GOLDEN, "keys_rsa2048.json")))["keys"][:n_keys]
    ks = [K.Key("rsa2048#%d" % i, int(k["p"], 16), int(k["q"], 16), int(k["e"], 16)) for i, k in enumerate(raw)]
    ds = [k.d() for k in ks]
    signed = []
    for j in range(200):
        ki = j % n_keys
        dg = rng.bytes(32)
        signed.append((ki, dg, pow(int.from_bytes(V.em(256, 8, dg), "big"), ds[ki], ks[ki].n)))
    digests, sigs, idx, expect = [], [], [], []
    for i in range(2000):
        ki, dg, s = signed[int(rng.integers(200))]
        ok = 1
        if i % 7 == 3:
            ok = 0
            if i % 2:
                s ^= 1 << int(rng.integers(2040))
            else:
                dg = bytes([dg[0] ^ 0x80]) + dg[1:]
        digests.append(dg); sigs.append(s.to_bytes(256, "big")); idx.append(ki); expect.append(ok)
    return [(k.n, k.e) for k in ks], digests, sigs, idx, np.array(expect, dtype=np.uint8)


@pytest.mark.parametrize("n_keys", [1, 100])
def test_two_thousand(gpu_ctx, n_keys):
    keys, digests, sigs, idx, expect = _volume(n_keys)
    valid, st = gpu_ctx.rsa_verify(digests, sigs, keys, 8, key_idx=None if n_keys == 1 else idx, nbytes=256)
    assert not st.any(), np.flatnonzero(st)[:8]
    assert (valid == expect).all(), np.flatnonzero(valid != expect)[:8]
    assert expect.sum() == 2000 - len(range(3, 2000, 7))
    rng = np.random.default_rng(16)
    for i in [int(v) for v in rng.choice(2000, 12, replace=False)] + [3, 10, 17, 24]:
        n, e = keys[idx[i]]
        assert (int(valid[i]), int(st[i])) == V.verify(n, e, 8, digests[i], int.from_bytes(sigs[i], "big")), i


def _raw(cases, nbytes=256):
    from bftkv_amd._native import _ints_to_be
    dg, sg, keys, idx = K.call_arrays(cases, nbytes)
    a = lambda b: np.frombuffer(b, dtype=np.uint8).copy()          # noqa: E731
    return dict(n=len(cases), dg=a(b"".join(dg)), hash_id=cases[0].hash_id, dlen=len(cases[0].digest), sg=a(b"".join(sg)), idx=idx, n_keys=len(keys),
                kn=_ints_to_be([k[0] for k in keys], nbytes), ke=np.array([k[1] for k in keys], dtype=np.uint32), nbytes=nbytes)


def test_device_form_against_host_form(rsav_ctx):
    import torch
    lib, h = rsav_ctx.lib, rsav_ctx.h
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")    # noqa: E731
    for cases in (fitting(K.corpus(0, 36))[:300], _pool()[:70], _pool()[:1]):
        a = _raw(cases)
        n = a["n"]
        exp = want(cases)
        d_dg, d_sg, d_ki = up(a["dg"]), up(a["sg"]), up(a["idx"].view(np.int32))
        d_valid = torch.full((n + 8,), 0x55, dtype=torch.uint8, device="cuda:0")
        d_st = torch.full((n + 8,), 0x55, dtype=torch.uint8, device="cuda:0")
        rsav_ctx._check(lib.bftkv_gpu_rsa_verify_dev(h, n, d_dg.data_ptr(), a["hash_id"], a["dlen"], d_sg.data_ptr(), 256, d_ki.data_ptr(), a["n_keys"],
                                                     P(a["kn"]), P(a["ke"]), d_valid.data_ptr(), d_st.data_ptr()), "rsa_verify_dev")
        rsav_ctx.sync()
        got = list(zip(d_valid.cpu().numpy()[:n].tolist(), d_st.cpu().numpy()[:n].tolist()))
        assert got == exp and got == call(rsav_ctx, cases)
        assert (d_valid.cpu().numpy()[n:] == 0x55).all() and (d_st.cpu().numpy()[n:] == 0x55).all()      # nothing past n_ops


def test_return_codes(gpu_ctx):
    lib, h = gpu_ctx.lib, gpu_ctx.h
    cases = [c for name in ("rsa1024", "rsa2048") for c in K.cell(name, 8, 32) if c.part in ("honest", "mutation")]
    a = _raw(cases)
    n = a["n"]

    def run(n_ops=n, dg=a["dg"], hash_id=8, dlen=32, sg=a["sg"], nb=256, idx=a["idx"], n_keys=a["n_keys"], kn=a["kn"], ke=a["ke"], out=True, ctx=h):
        valid, st = np.full(n + 4, 0xAA, dtype=np.uint8), np.full(n + 4, 0xAA, dtype=np.uint8)
        rc = lib.bftkv_gpu_rsa_verify(ctx, n_ops, P(dg), hash_id, dlen, P(sg), nb, P(idx), n_keys, P(kn), P(ke), P(valid) if out else None,
                                      P(st) if out else None)
        return rc, valid, st

    rc, valid, st = run()
    assert rc == 0 and [(int(v), int(s)) for v, s in zip(valid[:n], st[:n])] == want(cases)
    assert (valid[n:] == 0xAA).all() and (st[n:] == 0xAA).all()              # the canary behind the outputs
    rc, valid, st = run(n_ops=0)
    assert rc == 0 and (valid == 0xAA).all() and (st == 0xAA).all()
    assert lib.bftkv_gpu_rsa_verify(h, 0, None, 8, 32, None, 256, None, 1, P(a["kn"]), P(a["ke"]), None, None) == 0
    refused = [dict(hash_id=4), dict(hash_id=12), dict(hash_id=0xFFFFFFFF), dict(dlen=31), dict(dlen=0), dict(hash_id=2, dlen=32), dict(hash_id=0, dlen=65),
               dict(hash_id=0, dlen=0), dict(nb=0), dict(nb=257), dict(n_keys=0), dict(dg=None), dict(sg=None), dict(kn=None), dict(ke=None)]
    for kw in refused:
        rc, valid, st = run(**kw)
        assert rc == E_INVALID, (list(kw), rc)
        assert (st[:n] == FAILED).all() and (valid[:n] == 0).all(), list(kw)             # fail closed
        assert (valid[n:] == 0xAA).all() and (st[n:] == 0xAA).all()
    assert run(out=False)[0] == E_INVALID and run(ctx=None)[0] == E_INVALID
    # an even modulus refuses nothing: its signatures are fenced, the others answered
    even = a["kn"].copy()
    even[int(a["idx"][0]), -1] &= 0xFE
    rc, valid, st = run(kn=even)
    assert rc == 0 and (int(valid[0]), int(st[0])) == (0, V.FENCED)
    assert [(int(v), int(s)) for i, (v, s) in enumerate(zip(valid[:n], st[:n])) if a["idx"][i] != a["idx"][0]] == \
           [w for i, w in enumerate(want(cases)) if a["idx"][i] != a["idx"][0]]
    # the batcher: bad arguments fail closed for the caller alone
    from bftkv_amd import Batcher
    cs = next(c for c in cases if want([c]) == [(1, V.OK)])
    one = _raw([cs])
    v1, s1 = np.full(1, 0xAA, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
    bargs = lambda b, hash_id=8, dlen=32, nb=256: (b, P(one["dg"]), hash_id, dlen, P(one["sg"]), nb, P(one["kn"]), int(one["ke"][0]), P(v1), P(s1))    # noqa: E731
    assert lib.bftkv_gpu_batcher_rsa_verify(*bargs(None)) == E_INVALID and (int(v1[0]), int(s1[0])) == (0, FAILED)
    b = Batcher(gpu_ctx, max_items=8, n_lanes=1)
    for kw in (dict(dlen=31), dict(hash_id=5), dict(nb=0), dict(nb=300)):
        v1[0], s1[0] = 0xAA, 0
        assert lib.bftkv_gpu_batcher_rsa_verify(*bargs(b.h, **kw)) == E_INVALID and (int(v1[0]), int(s1[0])) == (0, FAILED), kw
    assert lib.bftkv_gpu_batcher_rsa_verify(*bargs(b.h)) == 0 and (int(v1[0]), int(s1[0])) == (1, V.OK)
    b.close()


def test_known_answer_of_the_reference(gpu_ctx):
    kat = json.load(open(os.path.join(K.GOLDEN, "threshold_kat.json")))["rsa"]
    n, e, sig = int(kat["n"], 16), int(kat["e"]), int(kat["sha256_pkcs1v15_sig"], 16)
    dg = hashlib.sha256(kat["tbs"].encode()).digest()
    valid, st = gpu_ctx.rsa_verify([dg, dg], [sig.to_bytes(256, "big"), (sig ^ 2).to_bytes(256, "big")], [(n, e)], 8)
    assert valid.tolist() == [1, 0] and not st.any()


def test_batcher_mixed(gpu_ctx):
    """64 threads, one signature per call: three modulus sizes, two hashes and hash id 0, valid, invalid and fenced mixed; one caller
    brings a wrong dlen and is refused alone."""
    from bftkv_amd import Batcher
    jobs = []
    for name in ("rsa1024", "rsa2048", "rsa752"):
        for cellid in ((8, 32), (10, 64), (0, 36)):
            jobs += [c for c in K.cell(name, *cellid) if c.part in ("honest", "mutation", "forgery", "key", "wide") and c.min_nbytes <= K.key(name).k]
    rng = np.random.default_rng(64)
    jobs = [jobs[int(i)] for i in rng.permutation(len(jobs))][:128]
    exp = want(jobs)
    assert set(exp) == {(1, V.OK), (0, V.OK), (0, V.FENCED)} and len({c.hash_id for c in jobs}) == 3
    b = Batcher(gpu_ctx, max_items=64, n_lanes=2)
    got = [None] * len(jobs)
    odd = {}

    def run(lo):
        for i in range(lo, len(jobs), 64):
            c = jobs[i]
            got[i] = b.rsa_verify(c.digest, c.s.to_bytes(K.key(c.key).k, "big"), c.n, c.e, c.hash_id)
        if lo == 5:
            c = jobs[lo]
            odd["dlen"] = b.rsa_verify(c.digest + b"\x00", c.s.to_bytes(K.key(c.key).k, "big"), c.n, c.e, c.hash_id or 8)

    th = [threading.Thread(target=run, args=(i,)) for i in range(64)]
    for t_ in th:
        t_.start()
    for t_ in th:
        t_.join()
    b.close()
    for i, (w, g) in enumerate(zip(exp, got)):
        assert g == (0, w[1], w[0]), (i, jobs[i].key, jobs[i].label, w, g)
    assert odd["dlen"] == (E_INVALID, FAILED, 0)
