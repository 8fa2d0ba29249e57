"""ECDSA-verification rates on the device: per curve, in one process and on one build,
  (a) 80,000 verifications under one key (bftkv_gpu_ecdsa_verify),
  (b) 80,000 bftkv_gpu_ec_scalar_base_mult calls -- the yardstick: one table-free scalar multiplication and one inversion each,
  (c) a lone verification,
for each window width of the fixed-base G table asked for (BFTKV_EC_WINDOW, one child process per width).  Times are a
synchronised host clock around the C calls on arrays prepared beforehand (median of --reps after a warm-up call); the
signatures are honest ones made from (b)'s own outputs, and every verdict is checked.

    python tools/ecdsa_verify_rate.py [--reps 3] [--windows 4,5,6] [--n 80000] [--out rate.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def median(ts):
    return sorted(ts)[len(ts) // 2]


def child(window: int, reps: int, n_ops: int):
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
    rng = np.random.default_rng(1)
    for name in E.NAMES:
        c = E.CURVES[name]
        n, f = c["n"], E.byte_len(c)
        cb, bits, _ = _curve_bytes(c)
        d = int.from_bytes(rng.bytes(80), "big") % n
        ks = [int.from_bytes(rng.bytes(80), "big") % n or 1 for _ in range(n_ops)]
        sc = _ints_to_be(ks + [d], f)
        pts = np.zeros((n_ops + 1, 1 + 2 * f), dtype=np.uint8)
        st = np.zeros(n_ops + 9, dtype=np.uint8)

        def base_mult(count):
            t0 = time.perf_counter()
            rc = lib.bftkv_gpu_ec_scalar_base_mult(h, count, P(sc), f, P(cb), bits, P(pts), P(st))
            t = time.perf_counter() - t0
            assert rc == 0 and not st[:count].any()
            return t

        base_mult(n_ops + 1)                                            # warm-up; also d G, the key, in the last row
        key = pts[n_ops].copy()
        t_b = median([base_mult(n_ops) for _ in range(reps)])
        dlen = min(f, 64)
        dg = np.frombuffer(rng.bytes(n_ops * dlen), dtype=np.uint8).reshape(n_ops, dlen).copy()
        sg = np.zeros((n_ops, 2 * f), dtype=np.uint8)
        for i in range(n_ops):
            r = int.from_bytes(pts[i, 1:1 + f].tobytes(), "big") % n
            s = pow(ks[i], -1, n) * (V.hash_to_int(c, dg[i].tobytes()) + r * d) % n
            sg[i] = np.frombuffer(r.to_bytes(f, "big") + s.to_bytes(f, "big"), dtype=np.uint8)
        sg[5, 2 * f - 1] ^= 1                                            # one forgery: the verdicts are not a constant
        valid = np.zeros(n_ops + 8, dtype=np.uint8)

        def verify(count):
            t0 = time.perf_counter()
            rc = lib.bftkv_gpu_ecdsa_verify(h, count, P(dg), dlen, P(sg), None, 1, P(key), P(cb), bits, P(valid), P(st))
            t = time.perf_counter() - t0
            assert rc == 0 and not st[:count].any()
            return t

        verify(n_ops)                                                   # warm-up: builds the curve's table
        assert valid[:n_ops].sum() == n_ops - 1 and valid[5] == 0
        t_a = median([verify(n_ops) for _ in range(reps)])
        t_c = median([verify(1) for _ in range(max(reps, 5))])
        out.append({"curve": name, "window": window or 4, "n": n_ops, "verify_ms": round(t_a * 1e3, 2), "base_mult_ms": round(t_b * 1e3, 2),
                    "ratio": round(t_a / t_b, 3), "verify_per_s": round(n_ops / t_a), "lone_verify_ms": round(t_c * 1e3, 3)})
    ctx.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--n", type=int, default=80000)
    ap.add_argument("--windows", default="4")
    ap.add_argument("--out")
    ap.add_argument("--child", type=int, default=-1)
    a = ap.parse_args()
    if a.child >= 0:
        child(a.child, a.reps, a.n)
        return
    res = {"kind": "device", "clock": "host, synchronised C calls, median of %d" % a.reps, "runs": []}
    for w in [int(v) for v in a.windows.split(",")]:
        env = dict(os.environ, BFTKV_EC_WINDOW=str(w))
        p = subprocess.run([sys.executable, __file__, "--child", str(w), "--reps", str(a.reps), "--n", str(a.n)], env=env, capture_output=True,
                           text=True, timeout=900)
        if p.returncode != 0:               # (a failed child ends the run: nothing more is started on the device)
            res["runs"].append({"window": w, "error": p.stderr[-2000:]})
            break
        res["runs"].extend(json.loads(p.stdout.strip().splitlines()[-1]))
    res["openssl"] = "not measured"
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
