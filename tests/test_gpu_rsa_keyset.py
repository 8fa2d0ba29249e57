"""GPU: resident RSA key sets (bftkv_gpu_rsa_keyset_* and bftkv_gpu_rsa_verify_keyset, its _dev form and the batcher kind): the same
answers as the raw entry for the same bytes, over the seeded corpus (tests/rsa_verify_cases.py)."""
import ctypes as C
import threading

import numpy as np
import pytest

import rsa_verify_cases as K
import rsa_verify_ref as V
from test_gpu_rsa_verify import CELL_IDS, FAILED, E_INVALID, P, fitting, rsav_ctx, want  # noqa: F401

pytestmark = pytest.mark.gpu
E_STATE = -5


def _set_call(ctx, ks, cases, nbytes=256):
    dg, sg, keys, idx = K.call_arrays(cases, nbytes)
    valid, st = ctx.rsa_verify_keyset(ks, dg, sg, cases[0].hash_id, key_idx=idx)
    return [(int(v), int(s)) for v, s in zip(valid, st)]


def test_answers_identical_to_the_raw_entry_on_the_whole_corpus(rsav_ctx):   # noqa: F811
    for cellid in K.HASH_CELLS:
        cases = fitting(K.corpus(*cellid))
        dg, sg, keys, idx = K.call_arrays(cases, 256)
        ks = rsav_ctx.rsa_keyset_create(keys, nbytes=256)
        info = rsav_ctx.rsa_keyset_info(ks)
        assert info == dict(n_keys=len(keys), n_refused=sum(1 for n, _ in keys if n % 2 == 0), nbytes=256) and info["n_refused"] >= 50
        got = _set_call(rsav_ctx, ks, cases)
        valid, st = rsav_ctx.rsa_verify(dg, sg, keys, cellid[0], key_idx=idx, nbytes=256)
        assert got == [(int(v), int(s)) for v, s in zip(valid, st)] and got == want(cases), cellid
        # a refused key is answered FENCED, or OK by row 1
        even = [g for g, c in zip(got, cases) if c.n % 2 == 0]
        assert set(even) <= {(0, V.FENCED), (0, V.OK)} and (0, V.FENCED) in even and (0, V.OK) in even
        rsav_ctx.rsa_keyset_destroy(ks)


def test_handles_forks_and_the_device_form(gpu_ctx):
    import torch
    lib = gpu_ctx.lib
    cases = [c for name in ("rsa1024", "rsa2048", "rsa496") for c in K.cell(name, 8, 32) if c.part in ("honest", "mutation", "key", "wide")]
    cases = fitting(cases)
    dg, sg, keys, idx = K.call_arrays(cases, 256)
    exp = want(cases)
    a = gpu_ctx.rsa_keyset_create(keys, nbytes=256)
    b = gpu_ctx.rsa_keyset_create(keys[:1], nbytes=256)
    assert a != b and _set_call(gpu_ctx, a, cases) == exp
    # NULL indices: key 0; an index past the set: its last key
    valid, st = gpu_ctx.rsa_verify_keyset(a, dg[:3], sg[:3], 8)
    assert [(int(v), int(s)) for v, s in zip(valid, st)] == [V.verify(*keys[0], 8, d, int.from_bytes(s_, "big")) for d, s_ in zip(dg[:3], sg[:3])]
    valid, st = gpu_ctx.rsa_verify_keyset(a, dg[:3], sg[:3], 8, key_idx=[len(keys), 0xFFFFFFFF, len(keys) - 1])
    assert [(int(v), int(s)) for v, s in zip(valid, st)] == [V.verify(*keys[-1], 8, d, int.from_bytes(s_, "big")) for d, s_ in zip(dg[:3], sg[:3])]
    # a fork reads the root's sets and may neither make nor retire one
    f = gpu_ctx.fork()
    assert _set_call(f, a, cases) == exp and f.rsa_keyset_info(b)["n_keys"] == 1
    h = C.c_int(-7)
    from bftkv_amd._native import _ints_to_be
    kn, ke = _ints_to_be([keys[0][0]], 256), np.array([keys[0][1]], dtype=np.uint32)
    assert lib.bftkv_gpu_rsa_keyset_create(f.h, 1, P(kn), P(ke), 256, C.byref(h)) == E_STATE and h.value == -7
    assert lib.bftkv_gpu_rsa_keyset_destroy(f.h, a) == E_STATE
    # the device form, with nothing written past n_ops
    n = len(cases)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")    # noqa: E731
    d_dg, d_sg = up(np.frombuffer(b"".join(dg), dtype=np.uint8).copy()), up(np.frombuffer(b"".join(sg), dtype=np.uint8).copy())
    d_ki = up(idx.view(np.int32))
    d_valid = torch.full((n + 8,), 0x55, dtype=torch.uint8, device="cuda:0")
    d_st = torch.full((n + 8,), 0x55, dtype=torch.uint8, device="cuda:0")
    f._check(lib.bftkv_gpu_rsa_verify_keyset_dev(f.h, a, n, d_dg.data_ptr(), 8, 32, d_sg.data_ptr(), d_ki.data_ptr(), d_valid.data_ptr(), d_st.data_ptr()),
             "rsa_verify_keyset_dev")
    f.sync()
    assert list(zip(d_valid.cpu().numpy()[:n].tolist(), d_st.cpu().numpy()[:n].tolist())) == exp
    assert (d_valid.cpu().numpy()[n:] == 0x55).all() and (d_st.cpu().numpy()[n:] == 0x55).all()
    f.close()
    # refusals fail closed; a destroyed handle is refused and handed out again
    valid, st = np.full(n + 4, 0xAA, dtype=np.uint8), np.full(n + 4, 0xAA, dtype=np.uint8)
    dgb, sgb = np.frombuffer(b"".join(dg), dtype=np.uint8).copy(), np.frombuffer(b"".join(sg), dtype=np.uint8).copy()
    for keyset, hash_id, dlen in ((99, 8, 32), (-1, 8, 32), (a, 8, 31), (a, 7, 32), (a, 0, 65)):
        valid[:], st[:] = 0xAA, 0xAA
        assert lib.bftkv_gpu_rsa_verify_keyset(gpu_ctx.h, keyset, n, P(dgb), hash_id, dlen, P(sgb), P(idx), P(valid), P(st)) == E_INVALID
        assert (valid[:n] == 0).all() and (st[:n] == FAILED).all() and (valid[n:] == 0xAA).all() and (st[n:] == 0xAA).all()
    assert lib.bftkv_gpu_rsa_verify_keyset(gpu_ctx.h, a, 0, None, 8, 32, None, None, None, None) == 0
    gpu_ctx.rsa_keyset_destroy(a)
    assert lib.bftkv_gpu_rsa_verify_keyset(gpu_ctx.h, a, n, P(dgb), 8, 32, P(sgb), P(idx), P(valid), P(st)) == E_INVALID and (st[:n] == FAILED).all()
    assert lib.bftkv_gpu_rsa_keyset_destroy(gpu_ctx.h, a) == E_INVALID and lib.bftkv_gpu_rsa_keyset_info(gpu_ctx.h, a, None, None, None) == E_INVALID
    assert gpu_ctx.rsa_keyset_info(b)["n_keys"] == 1
    a2 = gpu_ctx.rsa_keyset_create(keys, nbytes=256)
    assert a2 == a and _set_call(gpu_ctx, a2, cases) == exp
    for kw in (dict(n=0), dict(nb=0), dict(nb=257), dict(kn=None), dict(ke=None)):
        args = dict(n=1, kn=kn, ke=ke, nb=256)
        args.update(kw)
        assert lib.bftkv_gpu_rsa_keyset_create(gpu_ctx.h, args["n"], P(args["kn"]), P(args["ke"]), args["nb"], C.byref(h)) == E_INVALID and h.value == -7
    gpu_ctx.rsa_keyset_destroy(a2)
    gpu_ctx.rsa_keyset_destroy(b)


def test_handle_spaces_of_the_three_kinds_are_independent(gpu_ctx):
    """One set of each kind, each the smallest its own tests use.  Retiring the ECDSA set leaves the DSA and the RSA set answering,
    also where their handles have the retired one's number, and the next ECDSA set takes that number again."""
    import json
    import os
    import dsa_verify_cases as DK
    import dsa_verify_ref as DV
    import ec_ref as E
    lib, curve = gpu_ctx.lib, E.CURVES["P-256"]
    pts, pst = gpu_ctx.ec_scalar_base_mult([0x1234567], curve)
    assert not pst.any()
    k = json.load(open(os.path.join(DK.GOLDEN, "keys_dsa1024.json")))["keys"][0]
    p, q, g, x = (int(k[f], 16) for f in ("p", "q", "g", "x"))
    assert p.bit_length() == 1024 and q.bit_length() == 160
    rng = np.random.default_rng(8)
    ddg, rs = rng.bytes(20), None
    while rs is None:
        rs = DK.sign(p, q, g, x, ddg, DK.rnd(rng, q) or 1)
    assert DV.verify(p, q, g, pow(g, x, p), ddg, *rs) == (1, DV.OK)
    rcase = next(c for c in K.cell("rsa2048", 8, 32) if c.part == "honest" and want([c]) == [(1, V.OK)])
    e = gpu_ctx.ecdsa_keyset_create([pts[0]], curve)
    d = gpu_ctx.dsa_keyset_create([(0, pow(g, x, p))], [(p, q, g)], window_bits=4)
    r = gpu_ctx.rsa_keyset_create([(rcase.n, rcase.e)], nbytes=256)
    try:
        gpu_ctx.ecdsa_keyset_destroy(e)
        assert lib.bftkv_gpu_ecdsa_keyset_info(gpu_ctx.h, e, None, None, None, None) == E_INVALID
        assert gpu_ctx.dsa_keyset_info(d)["n_keys"] == 1 and gpu_ctx.dsa_keyset_info(d)["window_bits"] == 4
        assert gpu_ctx.rsa_keyset_info(r) == dict(n_keys=1, n_refused=0, nbytes=256)
        valid, st = gpu_ctx.dsa_verify_keyset(d, [ddg], [rs[0].to_bytes(20, "big") + rs[1].to_bytes(20, "big")])
        assert (int(valid[0]), int(st[0])) == (1, 0)
        valid, st = gpu_ctx.rsa_verify_keyset(r, [rcase.digest], [rcase.s.to_bytes(256, "big")], 8)
        assert (int(valid[0]), int(st[0])) == (1, 0)
        e2 = gpu_ctx.ecdsa_keyset_create([pts[0]], curve)
        assert e2 == e and gpu_ctx.ecdsa_keyset_info(e2)["n_keys"] == 1
        gpu_ctx.ecdsa_keyset_destroy(e2)
    finally:
        gpu_ctx.dsa_keyset_destroy(d)
        gpu_ctx.rsa_keyset_destroy(r)


def test_batcher_through_a_key_set(gpu_ctx):
    """64 threads, one signature per call under the keys of one set: three modulus sizes, two hashes and hash id 0, valid, invalid and
    fenced mixed; one caller with a wrong dlen and one with a dead handle are refused alone."""
    from bftkv_amd import Batcher
    jobs = []
    for name in ("rsa1024", "rsa2048", "rsa752"):
        for cellid in ((8, 32), (10, 64), (0, 36)):
            jobs += [c for c in K.cell(name, *cellid) if c.part in ("honest", "mutation", "forgery", "key", "wide") and c.min_nbytes <= 256]
    rng = np.random.default_rng(65)
    jobs = [jobs[int(i)] for i in rng.permutation(len(jobs))][:128]
    exp = want(jobs)
    assert set(exp) == {(1, V.OK), (0, V.OK), (0, V.FENCED)} and len({c.hash_id for c in jobs}) == 3
    _, _, keys, idx = K.call_arrays(jobs, 256)
    ks = gpu_ctx.rsa_keyset_create(keys, nbytes=256)
    b = Batcher(gpu_ctx, max_items=64, n_lanes=2)
    got = [None] * len(jobs)
    odd = {}

    def run(lo):
        for i in range(lo, len(jobs), 64):
            c = jobs[i]
            got[i] = b.rsa_verify_keyset(ks, int(idx[i]), c.digest, c.s.to_bytes(256, "big"), c.hash_id)
        c = jobs[lo]
        if lo == 5:
            odd["dlen"] = b.rsa_verify_keyset(ks, int(idx[lo]), c.digest + b"\x00", c.s.to_bytes(256, "big"), c.hash_id or 8)
        if lo == 9:
            v1, s1 = np.full(1, 0xAA, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
            dg, sg = np.frombuffer(c.digest, dtype=np.uint8).copy(), np.frombuffer(c.s.to_bytes(256, "big"), dtype=np.uint8).copy()
            rc = gpu_ctx.lib.bftkv_gpu_batcher_rsa_verify_keyset(b.h, ks + 40, 0, P(dg), c.hash_id, len(c.digest), P(sg), P(v1), P(s1))
            odd["handle"] = (rc, int(s1[0]), int(v1[0]))

    th = [threading.Thread(target=run, args=(i,)) for i in range(64)]
    for t_ in th:
        t_.start()
    for t_ in th:
        t_.join()
    b.close()
    gpu_ctx.rsa_keyset_destroy(ks)
    for i, (w, g) in enumerate(zip(exp, got)):
        assert g == (0, w[1], w[0]), (i, jobs[i].key, jobs[i].label, w, g)
    assert odd["dlen"] == (E_INVALID, FAILED, 0) and odd["handle"] == (E_INVALID, FAILED, 0)
