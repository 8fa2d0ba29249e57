"""GPU: raw RSA PKCS#1 v1.5 signing under resident private key sets against the restatement (tests/rsa_sign_ref.py) over the corpus
(tests/rsa_sign_cases.py): every status and every output byte.  Shapes are the smallest at which the kernels can still go wrong: every
key class under every hash id once, the operands at which the recombination can go wrong, one wave of eight different keys, and one
call of a launch's capacity + 17 under a 128-bit key."""
import ctypes as C
import random
import threading

import numpy as np
import pytest

import rsa_sign_cases as K
import rsa_sign_ref as R
import rsa_verify_ref as V
from bftkv_amd import Batcher, NativeError
from bftkv_amd._native import _ptr

pytestmark = pytest.mark.gpu
E_INVALID, E_STATE = -1, -5
LAUNCH = 16384
MIXED = ("rsa496", "rsa1024", "rsa2047", "rsa2048", "unbalanced", "kat", "full", "sparse")


@pytest.fixture(scope="module")
def signer(gpu_ctx):
    h = gpu_ctx.rsa_signer_create(K.key_dicts(), K.NBYTES, K.PBYTES)
    yield h
    gpu_ctx.rsa_signer_destroy(h)


@pytest.fixture(scope="module")
def small(gpu_ctx):
    """a second set: the 1024-bit and the 496-bit key in rows of 128 and 64 bytes"""
    ks = dict(K.keys())
    h = gpu_ctx.rsa_signer_create([ks["rsa1024"]._asdict(), ks["rsa496"]._asdict()], 128, 64)
    yield h
    gpu_ctx.rsa_signer_destroy(h)


def _small_want(tag, h, d):
    st, s = R.sign(dict(K.keys())[tag], h, d, 128)
    return st, s.to_bytes(128, "big")


def _compare(sig, st, want, what):
    assert len(st) == len(want)
    for j, (wst, wsig) in enumerate(want):
        assert st[j] == wst and sig[j].tobytes() == wsig, (what, j, int(st[j]), wst)


def test_set_info(gpu_ctx, signer, small):
    n_ref = sum(1 for t, _ in K.keys() if t.startswith("refused:"))
    assert gpu_ctx.rsa_signer_info(signer) == dict(n_keys=len(K.keys()), n_refused=n_ref, nbytes=K.NBYTES, pbytes=K.PBYTES) and n_ref == 8
    assert gpu_ctx.rsa_signer_info(small) == dict(n_keys=2, n_refused=0, nbytes=128, pbytes=64) and small != signer


@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: "hash%d_dlen%d" % s)
def test_corpus(gpu_ctx, signer, shape):
    digests, idx = K.call(*shape)
    sig, st = gpu_ctx.rsa_sign_keyset(signer, digests, shape[0], idx)
    _compare(sig, st, K.expected(*shape), shape)


def test_selftest_at_the_operands_where_the_recombination_can_go_wrong(gpu_ctx, signer):
    ops = K.selftest_ops()
    out, st = gpu_ctx.selftest_rsa_crt(signer, [c for _, _, c in ops], [i for i, _, _ in ops])
    for j, ((i, cls, _), (wst, ws)) in enumerate(zip(ops, K.selftest_expected())):
        assert st[j] == wst == R.OK and out[j].tobytes() == ws.to_bytes(K.NBYTES, "big"), (K.keys()[i][0], cls)
    # a refused key is fenced, and a value that does not fit the row is no answer: p q of 2048 bits under a registered n of 2040, in
    # rows of 255 bytes -- for the self-test and for a signature alike
    ref = next(i for i, (t, _) in enumerate(K.keys()) if t.startswith("refused:"))
    out, st = gpu_ctx.selftest_rsa_crt(signer, [5], [ref])
    assert st[0] == R.FENCED and not out.any()
    k = dict(K.keys())["rsa2048"]._replace(n=(1 << 2039) + 1)
    h255 = gpu_ctx.rsa_signer_create([k._asdict()], 255, 128)
    try:
        cs = [c for c in ((1 << 2039) - 1, 2, 3, 12345) if R.crt(k, c) >= 1 << 2040] + [1]
        out, st = gpu_ctx.selftest_rsa_crt(h255, cs)
        assert len(cs) > 1 and list(st) == [R.CHECK_FAILED] * (len(cs) - 1) + [R.OK] and not out[:-1].any() and out[-1].tobytes() == (1).to_bytes(255, "big")
        dg = [K.digest(8, 32, "wide %d" % j) for j in range(4)]
        assert all(R.crt(k, int.from_bytes(V.em(255, 8, x), "big")) >= 1 << 2040 for x in dg)
        sig, st = gpu_ctx.rsa_sign_keyset(h255, dg, 8)
        assert list(st) == [R.CHECK_FAILED] * 4 and not sig.any()
    finally:
        gpu_ctx.rsa_signer_destroy(h255)


def test_one_wave_of_eight_keys_of_different_sizes(gpu_ctx, signer):
    tags = [t for t, _ in K.keys()]
    order = list(MIXED)
    random.Random(8).shuffle(order)
    idx = [tags.index(t) for t in order]
    digests = [K.digest(8, 32, "mixed %d" % j) for j in range(8)]
    sig, st = gpu_ctx.rsa_sign_keyset(signer, digests, 8, idx)
    assert len({K.keys()[i][1].n.bit_length() for i in idx}) >= 5
    for j in range(8):
        one_sig, one_st = gpu_ctx.rsa_sign_keyset(signer, [digests[j]], 8, [idx[j]])
        want = R.sign(K.keys()[idx[j]][1], 8, digests[j], K.NBYTES)
        assert st[j] == one_st[0] == want[0] == R.OK and sig[j].tobytes() == one_sig[0].tobytes() == want[1].to_bytes(K.NBYTES, "big"), order[j]


def test_key_registry(gpu_ctx, signer, small):
    d = [K.digest(8, 32, "reg %d" % j) for j in range(4)]
    w1024, w496 = [_small_want("rsa1024", 8, x) for x in d], [_small_want("rsa496", 8, x) for x in d]
    _compare(*gpu_ctx.rsa_sign_keyset(small, d, 8, None), w1024, "key_idx NULL is key 0")
    _compare(*gpu_ctx.rsa_sign_keyset(small, d, 8, [0, 1, 2, 0xFFFFFFFF]), [w1024[0], w496[1], w496[2], w496[3]], "an index past the set is the last key")
    # two sets alive at once answer each for itself
    tags = [t for t, _ in K.keys()]
    sig, st = gpu_ctx.rsa_sign_keyset(signer, d[:1], 8, [tags.index("rsa1024")])
    assert st[0] == R.OK and sig[0, 128:].tobytes() == w1024[0][1] and not sig[0, :128].any()
    # a fork signs; it may neither create nor destroy
    f = gpu_ctx.fork()
    try:
        _compare(*f.rsa_sign_keyset(small, d, 8, [1, 1, 0, 0]), [w496[0], w496[1], w1024[2], w1024[3]], "fork")
        h = C.c_int(5)
        row = np.full((1, 8), 0xFF, dtype=np.uint8)
        e = np.array([3], dtype=np.uint32)
        assert f.lib.bftkv_gpu_rsa_signer_create(f.h, 1, _ptr(row), e.ctypes.data, 8, *[_ptr(row)] * 5, 8, C.byref(h)) == E_STATE and h.value == -1
        assert f.lib.bftkv_gpu_rsa_signer_destroy(f.h, small) == E_STATE
        assert f.rsa_signer_info(small)["n_keys"] == 2
    finally:
        f.close()
    # a destroyed handle is refused and handed out again
    ks = dict(K.keys())
    h2 = gpu_ctx.rsa_signer_create([ks["rsa496"]._asdict()], 62, 31)
    assert h2 not in (signer, small)
    gpu_ctx.rsa_signer_destroy(h2)
    sig, st = np.full((1, 62), 0xA5, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
    dg = np.frombuffer(d[0], dtype=np.uint8).copy()
    assert gpu_ctx.lib.bftkv_gpu_rsa_sign_keyset(gpu_ctx.h, h2, 1, _ptr(dg), 8, 32, None, _ptr(sig), _ptr(st)) == E_INVALID and st[0] == R.FAILED
    assert gpu_ctx.lib.bftkv_gpu_rsa_signer_destroy(gpu_ctx.h, h2) == E_INVALID
    with pytest.raises(NativeError):
        gpu_ctx.rsa_signer_info(h2)
    h3 = gpu_ctx.rsa_signer_create([ks["rsa496"]._asdict()], 62, 31)
    try:
        assert h3 == h2
        sig, st = gpu_ctx.rsa_sign_keyset(h3, d[:1], 8)
        assert st[0] == R.OK and sig[0].tobytes() == R.sign(ks["rsa496"], 8, d[0], 62)[1].to_bytes(62, "big")
    finally:
        gpu_ctx.rsa_signer_destroy(h3)


def test_call_level_refusals(gpu_ctx, signer):
    lib, h = gpu_ctx.lib, gpu_ctx.h
    dg = np.full((3, 64), 0x11, dtype=np.uint8)

    def call(handle, n, hash_id, dlen, digests=dg, null_out=False):
        sig, st = np.full((3, K.NBYTES), 0xA5, dtype=np.uint8), np.zeros(3, dtype=np.uint8)
        rc = lib.bftkv_gpu_rsa_sign_keyset(h, handle, n, None if digests is None else _ptr(digests), hash_id, dlen, None, None if null_out else _ptr(sig), _ptr(st))
        return rc, sig, st
    for what, args in (("unknown hash id", (signer, 3, 4, 32)), ("dlen is not the hash's size", (signer, 3, 8, 31)), ("hash id 0 with dlen 0", (signer, 3, 0, 0)),
                       ("hash id 0 with dlen 65", (signer, 3, 0, 65)), ("NULL digests", (signer, 3, 8, 32, None))):
        rc, sig, st = call(*args)
        assert rc == E_INVALID and (st == R.FAILED).all() and not sig.any(), what
    rc, sig, st = call(9999, 3, 8, 32)
    assert rc == E_INVALID and (st == R.FAILED).all()
    rc, sig, st = call(signer, 3, 8, 32, dg, True)
    assert rc == E_INVALID and (st == R.FAILED).all()
    rc, sig, st = call(signer, 0, 8, 32)                             # an empty call writes nothing
    assert rc == 0 and (sig == 0xA5).all() and not st.any()
    rc, sig, st = call(signer, 2, 8, 32)                             # nothing past n_ops
    assert rc == 0 and (sig[2] == 0xA5).all() and st[2] == 0 and list(st[:2]) == [R.INVALID_INPUT] * 2 and not sig[:2].any()      # key 0: 128 bits


def test_device_form_writes_nothing_past_n_ops(gpu_ctx, signer):
    import torch
    digests, idx = K.call(8, 32)
    n = len(digests)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")    # noqa: E731
    d_dg = up(np.frombuffer(b"".join(digests), dtype=np.uint8).copy())
    d_ki = up(np.array(idx, dtype=np.uint32).view(np.int32))
    d_sig = torch.full(((n + 8) * K.NBYTES,), 0x55, dtype=torch.uint8, device="cuda:0")
    d_st = torch.full((n + 8,), 0x55, dtype=torch.uint8, device="cuda:0")
    gpu_ctx._check(gpu_ctx.lib.bftkv_gpu_rsa_sign_keyset_dev(gpu_ctx.h, signer, n, d_dg.data_ptr(), 8, 32, d_ki.data_ptr(), d_sig.data_ptr(), d_st.data_ptr()),
                   "rsa_sign_keyset_dev")
    torch.cuda.synchronize()
    sig, st = d_sig.cpu().numpy().reshape(n + 8, K.NBYTES), d_st.cpu().numpy()
    _compare(sig[:n], st[:n], K.expected(8, 32), "dev")
    assert (sig[n:] == 0x55).all() and (st[n:] == 0x55).all()
    # a refused device call fails closed on the stream
    assert gpu_ctx.lib.bftkv_gpu_rsa_sign_keyset_dev(gpu_ctx.h, signer, n, d_dg.data_ptr(), 8, 31, d_ki.data_ptr(), d_sig.data_ptr(), d_st.data_ptr()) == E_INVALID
    torch.cuda.synchronize()
    sig, st = d_sig.cpu().numpy().reshape(n + 8, K.NBYTES), d_st.cpu().numpy()
    assert not sig[:n].any() and (st[:n] == R.FAILED).all() and (sig[n:] == 0x55).all() and (st[n:] == 0x55).all()


def test_more_signatures_than_one_launch_takes(gpu_ctx):
    """the launch's capacity + 17, made cheap: a 128-bit key in rows of 16 bytes, 8-byte private parts, hash id 0, dlen 4"""
    k = K.small_key()
    h = gpu_ctx.rsa_signer_create([k._asdict()], 16, 8)
    try:
        n = LAUNCH + 17
        rng = random.Random(17)
        digests = [rng.getrandbits(32).to_bytes(4, "big") for _ in range(n)]
        sig, st = gpu_ctx.rsa_sign_keyset(h, digests, 0)
        d = pow(k.e, -1, (k.p - 1) * (k.q - 1))
        want = np.frombuffer(b"".join(pow(int.from_bytes(V.em(16, 0, x), "big"), d, k.n).to_bytes(16, "big") for x in digests), dtype=np.uint8).reshape(n, 16)
        assert not st.any() and (sig == want).all(), np.nonzero((sig != want).any(axis=1))[0][:8]
        assert R.sign(k, 0, digests[-1], 16) == (R.OK, int.from_bytes(want[-1].tobytes(), "big"))
    finally:
        gpu_ctx.rsa_signer_destroy(h)


def test_the_verifier_accepts_every_signature_the_device_made(gpu_ctx, signer):
    digests, idx = K.call(8, 32)
    sig, st = gpu_ctx.rsa_sign_keyset(signer, digests, 8, idx)
    vk = gpu_ctx.rsa_keyset_create([(k.n, k.e) for _, k in K.keys()], K.NBYTES)
    try:
        valid, vst = gpu_ctx.rsa_verify_keyset(vk, digests, [s.tobytes() for s in sig], 8, idx)
        ok = st == R.OK
        assert ok.sum() > 30 and (valid[ok] == 1).all() and not valid[~ok].any() and not vst[ok].any()
    finally:
        gpu_ctx.rsa_keyset_destroy(vk)


def test_batcher(gpu_ctx, signer, small):
    """32 threads x 8 calls over two sets and two hash ids, mixed with verifications: every caller gets its own answer"""
    tags = [t for t, _ in K.keys()]
    big_keys = [tags.index(t) for t in MIXED] + [tags.index("broken:dq+1:rsa1024"), tags.index("refused:even_p:rsa496")]
    vk = gpu_ctx.rsa_keyset_create([(k.n, k.e) for _, k in K.keys()], K.NBYTES)
    plan, want = {}, {}
    rng = random.Random(32)
    for t in range(32):
        for c in range(8):
            h = (8, 2)[rng.randrange(2)]
            d = K.digest(h, V.DLEN[h], "batcher %d %d" % (t, c))
            which = rng.randrange(3)
            if which == 0:
                i = rng.choice(big_keys)
                st, s = R.sign(K.keys()[i][1], h, d, K.NBYTES)
                plan[(t, c)], want[(t, c)] = ("sign", signer, i, d, h), (0, st, s.to_bytes(K.NBYTES, "big"))
            elif which == 1:
                i = rng.randrange(2)
                plan[(t, c)], want[(t, c)] = ("sign", small, i, d, h), (0,) + _small_want(("rsa1024", "rsa496")[i], h, d)
            else:
                i = tags.index("rsa1024")
                s = R.sign(K.keys()[i][1], h, d, K.NBYTES)[1] ^ (c & 1)
                plan[(t, c)], want[(t, c)] = ("verify", vk, i, d, h, s.to_bytes(K.NBYTES, "big")), (0, 0, 1 - (c & 1))
    b = Batcher(gpu_ctx, max_items=64, max_wait_us=5000, n_lanes=2)
    got = {}
    gate = threading.Barrier(32)

    def run(t):
        gate.wait()
        for c in range(8):
            p = plan[(t, c)]
            if p[0] == "sign":
                got[(t, c)] = b.rsa_sign_keyset(p[1], p[2], p[3], p[4])
            else:
                got[(t, c)] = b.rsa_verify_keyset(p[1], p[2], p[3], p[5], p[4])
    th = [threading.Thread(target=run, args=(t,)) for t in range(32)]
    try:
        for x in th:
            x.start()
        for x in th:
            x.join()
        stats = b.stats()
        for key in plan:
            assert tuple(got[key]) == want[key], (key, plan[key][:3], got[key][:2], want[key][:2])
        assert {w[1] for w in want.values()} >= {R.OK, R.CHECK_FAILED, R.FENCED}
        assert stats["calls"] == 256 and stats["batches"] < 256 and stats["max_batch"] > 1, stats
        # call-level refusals, for the caller alone: as for the direct entry
        d = K.digest(8, 32, "refusal")
        for what, (handle, dg, hash_id) in (("unknown hash id", (signer, d, 4)), ("dlen is not the hash's size", (signer, d[:31], 8)), ("a bad handle", (9999, d, 8))):
            dga, sig, st = np.frombuffer(dg, dtype=np.uint8).copy(), np.full(K.NBYTES, 0xA5, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
            rc = gpu_ctx.lib.bftkv_gpu_batcher_rsa_sign_keyset(b.h, handle, 0, _ptr(dga), len(dg), hash_id, _ptr(sig), _ptr(st))
            assert rc == E_INVALID and st[0] == R.FAILED, what
        assert b.rsa_sign_keyset(small, 0, d, 8) == (0,) + _small_want("rsa1024", 8, d)
    finally:
        b.close()
        gpu_ctx.rsa_keyset_destroy(vk)


def test_the_same_call_twice_with_failures_in_between(gpu_ctx, signer):
    tags = [t for t, _ in K.keys()]
    digests, idx = K.call(2, 20)
    first = gpu_ctx.rsa_sign_keyset(signer, digests, 2, idx)
    _compare(*first, K.expected(2, 20), "first")
    dg = np.full((2, 20), 0x22, dtype=np.uint8)
    sig, st = np.full((2, K.NBYTES), 0xA5, dtype=np.uint8), np.zeros(2, dtype=np.uint8)
    assert gpu_ctx.lib.bftkv_gpu_rsa_sign_keyset(gpu_ctx.h, signer, 2, _ptr(dg), 2, 19, None, _ptr(sig), _ptr(st)) == E_INVALID     # a failing call
    bad = tags.index("broken:qinv+1:rsa2048")
    s2, st2 = gpu_ctx.rsa_sign_keyset(signer, digests[:3], 2, [bad] * 3)                                                            # a key that fails the check
    assert list(st2) == [R.CHECK_FAILED] * 3 and not s2.any()
    second = gpu_ctx.rsa_sign_keyset(signer, digests, 2, idx)
    assert second[0].tobytes() == first[0].tobytes() and second[1].tobytes() == first[1].tobytes()
