"""Resident ECDSA key sets against the raw entry on the device: per curve, in one process and on one build,
  (a) --n (80,000) verifications under ONE key,
  (b) --n verifications under --keys (1,000) keys chosen uniformly at random per signature (no sorting by key),
      each through bftkv_gpu_ecdsa_verify (the yardstick: key bytes in the call, u2 Q by the ladder) and through
      bftkv_gpu_ecdsa_verify_keyset (u2 Q from the key's table), the two ALTERNATING for --reps repetitions each,
  (c) the time bftkv_gpu_ecdsa_keyset_create takes for a set of 1 key and of --keys keys,
  (d) a lone verification through both entries.
Times are a synchronised host clock around the C calls on arrays prepared beforehand, after a warm-up call for every shape;
median, minimum and maximum are reported.  The signatures are honest ones (k G and d G from the device's ScalarBaseMult) with one
forgery each, and every verdict of every timed call is checked.  "faster_beyond_spread": the key set's slowest repetition of (a)
beats the raw entry's fastest one, i.e. the medians differ by more than the run-to-run spread of either.

    python tools/ecdsa_keyset_rate.py [--reps 5] [--n 80000] [--keys 1000] [--curves P-224,P-256,P-384,P-521] [--out rate.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(ts[len(ts) // 2] * 1e3, 3), "min_ms": round(ts[0] * 1e3, 3), "max_ms": round(ts[-1] * 1e3, 3)}


def run(names, reps, n_ops, n_keys):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import ec_ref as E
    import ecdsa_verify_ref as V
    from bftkv_amd import Context
    from bftkv_amd._native import _curve_bytes, _ints_to_be
    ctx = Context(0)
    lib, h = ctx.lib, ctx.h
    P = lambda a: a.ctypes.data_as(C.c_void_p)        # noqa: E731
    out = []
    rng = np.random.default_rng(2)
    for name in names:
        c = E.CURVES[name]
        n, f = c["n"], E.byte_len(c)
        cb, bits, _ = _curve_bytes(c)
        ds = [int.from_bytes(rng.bytes(80), "big") % n or 1 for _ in range(n_keys)]
        ks = [int.from_bytes(rng.bytes(80), "big") % n or 1 for _ in range(n_ops)]
        pts, st = ctx.ec_scalar_base_mult(ds + ks, c)
        assert not st.any()
        keys = np.frombuffer(b"".join(pts[:n_keys]), dtype=np.uint8).reshape(n_keys, 1 + 2 * f).copy()
        dlen = min(f, 64)
        dg = np.frombuffer(rng.bytes(n_ops * dlen), dtype=np.uint8).reshape(n_ops, dlen).copy()
        idx = rng.integers(n_keys, size=n_ops).astype(np.uint32)
        sg_one, sg_many = np.zeros((n_ops, 2 * f), dtype=np.uint8), np.zeros((n_ops, 2 * f), dtype=np.uint8)
        for i in range(n_ops):
            r = int.from_bytes(pts[n_keys + i][1:1 + f], "big") % n
            e, kinv = V.hash_to_int(c, dg[i].tobytes()), pow(ks[i], -1, n)
            rb = r.to_bytes(f, "big")
            sg_one[i] = np.frombuffer(rb + (kinv * (e + r * ds[0]) % n).to_bytes(f, "big"), dtype=np.uint8)
            sg_many[i] = np.frombuffer(rb + (kinv * (e + r * ds[int(idx[i])]) % n).to_bytes(f, "big"), dtype=np.uint8)
        for sg in (sg_one, sg_many):
            sg[5, 2 * f - 1] ^= 1                                        # one forgery: the verdicts are not a constant
        valid, stb = np.zeros(n_ops + 8, dtype=np.uint8), np.zeros(n_ops + 8, dtype=np.uint8)

        def checked(rc, count):
            assert rc == 0 and not stb[:count].any(), (name, rc)
            assert valid[:count].sum() == count - (1 if count > 5 else 0) and (count <= 5 or valid[5] == 0), name

        def raw(count, sg, ki, nk):
            t0 = time.perf_counter()
            rc = lib.bftkv_gpu_ecdsa_verify(h, count, P(dg), dlen, P(sg), None if ki is None else P(ki), nk, P(keys), P(cb), bits, P(valid), P(stb))
            t = time.perf_counter() - t0
            checked(rc, count)
            return t

        def through_set(handle, count, sg, ki):
            t0 = time.perf_counter()
            rc = lib.bftkv_gpu_ecdsa_verify_keyset(h, handle, count, P(dg), dlen, P(sg), None if ki is None else P(ki), P(valid), P(stb))
            t = time.perf_counter() - t0
            checked(rc, count)
            return t

        def create(nk):
            hs = C.c_int(-1)
            t0 = time.perf_counter()
            rc = lib.bftkv_gpu_ecdsa_keyset_create(h, nk, P(keys), P(cb), bits, C.byref(hs))
            t = time.perf_counter() - t0
            assert rc == 0, (name, rc)
            return t, hs.value

        row = {"curve": name, "n": n_ops, "keys": n_keys, "reps": reps}
        # (c) creation, after one warm-up creation (the context's G table, N's rows and the kernels' code objects)
        ctx.ecdsa_keyset_destroy(create(1)[1])
        t_c1, t_cn = [], []
        for _ in range(3):
            for ts, nk in ((t_c1, 1), (t_cn, n_keys)):
                t, hs = create(nk)
                ts.append(t)
                ctx.ecdsa_keyset_destroy(hs)
        row["create_1_key"], row["create_%d_keys" % n_keys] = stats(t_c1), stats(t_cn)
        one, many = create(1)[1], create(n_keys)[1]
        info = ctx.ecdsa_keyset_info(many)
        row["window_bits"], row["table_bytes_%d_keys" % n_keys] = info["window_bits"], info["table_bytes"]
        assert info["n_refused"] == 0
        # (a) and (b): warm-up for every shape, then the two entries alternating
        for label, sg, ki, nk, handle in (("one_key", sg_one, None, 1, one), ("%d_keys" % n_keys, sg_many, idx, n_keys, many)):
            raw(n_ops, sg, ki, nk)
            through_set(handle, n_ops, sg, ki)
            t_raw, t_set = [], []
            for _ in range(reps):
                t_raw.append(raw(n_ops, sg, ki, nk))
                t_set.append(through_set(handle, n_ops, sg, ki))
            r_, s_ = stats(t_raw), stats(t_set)
            row[label] = {"raw": r_, "keyset": s_, "raw_over_keyset": round(r_["median_ms"] / s_["median_ms"], 3),
                          "raw_per_s": round(n_ops / (r_["median_ms"] * 1e-3)), "keyset_per_s": round(n_ops / (s_["median_ms"] * 1e-3)),
                          "faster_beyond_spread": s_["max_ms"] < r_["min_ms"]}
        # (d) a lone verification
        raw(1, sg_one, None, 1)
        through_set(one, 1, sg_one, None)
        t_raw, t_set = [], []
        for _ in range(max(reps, 9)):
            t_raw.append(raw(1, sg_one, None, 1))
            t_set.append(through_set(one, 1, sg_one, None))
        row["lone"] = {"raw": stats(t_raw), "keyset": stats(t_set)}
        ctx.ecdsa_keyset_destroy(one)
        ctx.ecdsa_keyset_destroy(many)
        print(json.dumps(row), file=sys.stderr, flush=True)
        out.append(row)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=80000)
    ap.add_argument("--keys", type=int, default=1000)
    ap.add_argument("--curves", default="P-224,P-256,P-384,P-521")
    ap.add_argument("--out")
    a = ap.parse_args()
    res = {"kind": "device", "clock": "host, synchronised C calls; raw entry and key set alternating, %d repetitions each after a warm-up" % a.reps,
           "command": "python tools/ecdsa_keyset_rate.py --reps %d --n %d --keys %d --curves %s" % (a.reps, a.n, a.keys, a.curves),
           "runs": run(a.curves.split(","), a.reps, a.n, a.keys)}
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
