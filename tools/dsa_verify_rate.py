"""DSA-verification rates on the device: 10,000 raw signatures under the groups of tests/golden/keys_dsa2048.json and
keys_dsa1024.json, under one key and under 100 keys (key i in group i modulo the file's groups), for each lane form of k_dsav_exp
(BFTKV_MULTIEXP_LANES = 4 and 8, one child process per form).  Timed with events on the context's stream around the _dev entry
(arrays resident, after a warm-up call; median of --reps), with the host form's wall time beside it; every verdict is checked.
The first child also times OpenSSL's DSA_do_verify on 16 host threads over the same batches (objects built beforehand).

    python tools/dsa_verify_rate.py [--reps 5] [--n 10000] [--out profiles/dsa_verify_rate.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_THREADS = 16


def median(ts):
    return sorted(ts)[len(ts) // 2]


def openssl_rate(groups, keys, key_idx, digests, rs):
    """Seconds DSA_do_verify takes over the batch on HOST_THREADS threads (ctypes drops the GIL inside the call), or None."""
    try:
        lib = C.CDLL("libcrypto.so.3")
    except OSError:
        return None
    vp = C.c_void_p
    for name, res, args in [("DSA_new", vp, []), ("DSA_set0_pqg", C.c_int, [vp, vp, vp, vp]), ("DSA_set0_key", C.c_int, [vp, vp, vp]),
                            ("BN_bin2bn", vp, [C.c_char_p, C.c_int, vp]), ("DSA_SIG_new", vp, []), ("DSA_SIG_set0", C.c_int, [vp, vp, vp]),
                            ("DSA_do_verify", C.c_int, [C.c_char_p, C.c_int, vp, vp])]:
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args

    def bn(v):
        b = v.to_bytes((v.bit_length() + 7) // 8 or 1, "big")
        return lib.BN_bin2bn(b, len(b), None)
    dsas = []
    for gi, y in keys:
        d = lib.DSA_new()
        p, q, g = groups[gi]
        assert lib.DSA_set0_pqg(d, bn(p), bn(q), bn(g)) == 1 and lib.DSA_set0_key(d, bn(y), None) == 1
        dsas.append(d)
    sigs = []
    for r, s in rs:
        sg = lib.DSA_SIG_new()
        assert lib.DSA_SIG_set0(sg, bn(r), bn(s)) == 1
        sigs.append(sg)
    n = len(rs)

    def part(t):
        ok = 0
        for i in range(t, n, HOST_THREADS):
            ok += lib.DSA_do_verify(digests[i], len(digests[i]), sigs[i], dsas[key_idx[i]]) == 1
        return ok
    with ThreadPoolExecutor(HOST_THREADS) as ex:
        list(ex.map(part, range(HOST_THREADS)))                         # warm-up (Montgomery contexts are cached per key)
        t0 = time.perf_counter()
        good = sum(ex.map(part, range(HOST_THREADS)))
        t = time.perf_counter() - t0
    assert good == n - 1                                                # (objects are left to the process's end)
    return t


def child(lanes: int, reps: int, n_ops: int, with_openssl: bool):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from bftkv_amd import Context
    from bftkv_amd._native import _ints_to_be
    ctx = Context(0)
    lib, h = ctx.lib, ctx.h
    stream = torch.cuda.ExternalStream(int(lib.bftkv_gpu_stream(h)))
    P = lambda a: a.ctypes.data_as(C.c_void_p)        # noqa: E731
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")    # noqa: E731
    rng = np.random.default_rng(1)
    out = []
    for kind in ("dsa2048", "dsa1024"):
        file_keys = json.load(open(os.path.join(ROOT, "tests", "golden", "keys_%s.json" % kind)))["keys"]
        for n_keys in (1, 100):
            groups, keys, xs = [], [], []
            for i in range(n_keys):
                e = file_keys[i % len(file_keys)]
                p, q, g = (int(e[f], 16) for f in ("p", "q", "g"))
                if (p, q, g) not in groups:
                    groups.append((p, q, g))
                x = int(e["x"], 16) if i < len(file_keys) else int.from_bytes(rng.bytes(40), "big") % q or 1
                keys.append((groups.index((p, q, g)), pow(g, x, p)))
                xs.append(x)
            qb = (groups[0][1].bit_length() + 7) // 8
            key_idx = [int(v) for v in rng.integers(n_keys, size=n_ops)]
            ks = [int.from_bytes(rng.bytes(40), "big") % groups[keys[k][0]][1] or 1 for k in key_idx]
            # r = g^k mod p mod q with the power from the device (CalculatePartialR's kernel), s on the host
            gk = ctx.modexp_ops(_ints_to_be([groups[keys[k][0]][2] for k in key_idx], 256), np.array([keys[k][0] for k in key_idx], dtype=np.uint32),
                                _ints_to_be([g_[0] for g_ in groups], 256), _ints_to_be(ks, 32))
            digests = [rng.bytes(qb) for _ in range(n_ops)]
            rs = []
            for i in range(n_ops):
                q = groups[keys[key_idx[i]][0]][1]
                r = int.from_bytes(gk[i].tobytes(), "big") % q
                s = pow(ks[i], -1, q) * (int.from_bytes(digests[i], "big") + xs[key_idx[i]] * r) % q
                rs.append((r, s))
            rs[5] = (rs[5][0], rs[5][1] ^ 1)                             # one forgery: the verdicts are not a constant
            dg = np.frombuffer(b"".join(digests), dtype=np.uint8).copy()
            sg = np.frombuffer(b"".join(r.to_bytes(qb, "big") + s.to_bytes(qb, "big") for r, s in rs), dtype=np.uint8).copy()
            ki = np.array(key_idx, dtype=np.uint32)
            y, kg = _ints_to_be([k[1] for k in keys], 256), np.array([k[0] for k in keys], dtype=np.uint32)
            p_, q_, g_ = (_ints_to_be([t[j] for t in groups], w) for j, w in ((0, 256), (1, qb), (2, 256)))
            tail = (n_keys, P(y), P(kg), 256, len(groups), P(p_), P(q_), P(g_))
            valid, st = np.zeros(n_ops, dtype=np.uint8), np.zeros(n_ops, dtype=np.uint8)

            def host_call():
                t0 = time.perf_counter()
                rc = lib.bftkv_gpu_dsa_verify(h, n_ops, P(dg), qb, P(sg), qb, P(ki), *tail, P(valid), P(st))
                t = time.perf_counter() - t0
                assert rc == 0 and not st.any() and valid.sum() == n_ops - 1 and valid[5] == 0
                return t

            host_call()                                                  # warm-up: Montgomery rows into the context's cache
            t_host = median([host_call() for _ in range(reps)])
            d_dg, d_sg, d_ki = up(dg), up(sg), up(ki.view(np.int32))
            d_valid, d_st = torch.zeros(n_ops, dtype=torch.uint8, device="cuda:0"), torch.zeros(n_ops, dtype=torch.uint8, device="cuda:0")

            def dev_call():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                rc = lib.bftkv_gpu_dsa_verify_dev(h, n_ops, d_dg.data_ptr(), qb, d_sg.data_ptr(), qb, d_ki.data_ptr(), *tail, d_valid.data_ptr(),
                                                  d_st.data_ptr())
                e1.record(stream)
                e1.synchronize()
                assert rc == 0
                return e0.elapsed_time(e1) * 1e-3

            dev_call()
            assert int(d_valid.sum()) == n_ops - 1 and not bool(d_st.any())
            t_dev = median([dev_call() for _ in range(reps)])
            row = {"group": kind, "n_keys": n_keys, "n_groups": len(groups), "lanes": lanes, "n": n_ops, "events_ms": round(t_dev * 1e3, 3),
                   "events_per_s": round(n_ops / t_dev), "host_call_ms": round(t_host * 1e3, 3), "host_call_per_s": round(n_ops / t_host)}
            if with_openssl:
                t_o = openssl_rate(groups, keys, key_idx, digests, rs)
                row["openssl_16_threads_ms"] = None if t_o is None else round(t_o * 1e3, 2)
                row["openssl_16_threads_per_s"] = None if t_o is None else round(n_ops / t_o)
            out.append(row)
    ctx.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--out")
    ap.add_argument("--child", type=int, default=-1)
    ap.add_argument("--openssl", action="store_true")
    a = ap.parse_args()
    if a.child >= 0:
        child(a.child, a.reps, a.n, a.openssl)
        return
    res = {"kind": "device", "clock": "events on the context's stream around the _dev entry, median of %d; host_call = wall time of the host form" % a.reps,
           "openssl": "DSA_do_verify over the same batch on %d host threads" % HOST_THREADS, "runs": []}
    for i, lanes in enumerate((4, 8)):
        env = dict(os.environ, BFTKV_MULTIEXP_LANES=str(lanes))
        cmd = [sys.executable, __file__, "--child", str(lanes), "--reps", str(a.reps), "--n", str(a.n)] + (["--openssl"] if i == 0 else [])
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:               # (a failed child ends the run: nothing more is started on the device)
            res["runs"].append({"lanes": lanes, "error": p.stderr[-2000:]})
            break
        res["runs"].extend(json.loads(p.stdout.strip().splitlines()[-1]))
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
