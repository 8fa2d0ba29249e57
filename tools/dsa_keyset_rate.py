"""Resident DSA key sets against the raw entry on the device: per group (the first key of keys_dsa1024 / dsa1536 / dsa2048.json) and
per window width, in one process and on one build,
  (a) --n (80,000) verifications under ONE key,
  (b) --n verifications under --keys (1,000) keys of that group chosen uniformly at random per signature (no sorting by key),
      each through bftkv_gpu_dsa_verify (the yardstick: groups and keys in the call, 4-bit Straus; its code is unchanged) and
      through bftkv_gpu_dsa_verify_keyset (a chain of table products), the two ALTERNATING for --reps repetitions each,
  (c) the time bftkv_gpu_dsa_keyset_create takes for a set of 1 key and of --keys keys,
  (d) a lone verification through both entries.
Times are a synchronised host clock around the C calls on arrays prepared beforehand, after a warm-up call for every shape;
median, minimum and maximum are reported.  The signatures are honest ones (g^k and y = g^x from the device's modexp) with one
forgery each, and every verdict of every timed call is checked.  "faster_beyond_spread": the key set's slowest repetition of (a)
beats the raw entry's fastest one, i.e. the medians differ by more than the run-to-run spread of either.  A width whose tables
the device cannot hold is reported as "not measured".

    python tools/dsa_keyset_rate.py [--reps 5] [--n 80000] [--keys 1000] [--groups dsa1024,dsa1536,dsa2048] [--widths 4,8,12] [--out rate.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PB, QB = 256, 32          # the widths of every call: p, g, y in 256 bytes, q, r, s in 32
E_NOMEM = -3


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(ts[len(ts) // 2] * 1e3, 3), "min_ms": round(ts[0] * 1e3, 3), "max_ms": round(ts[-1] * 1e3, 3)}


def run(names, widths, reps, n_ops, n_keys):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    from bftkv_amd import Context
    from bftkv_amd._native import _ints_to_be
    ctx = Context(0)
    lib, h = ctx.lib, ctx.h
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)        # noqa: E731
    golden = os.path.join(ROOT, "tests", "golden")
    out = []
    rng = np.random.default_rng(3)
    for name in names:
        k0 = json.load(open(os.path.join(golden, "keys_%s.json" % name)))["keys"][0]
        p, q, g = (int(k0[f], 16) for f in ("p", "q", "g"))
        dlen = q.bit_length() // 8
        rnd = lambda: int.from_bytes(rng.bytes(40), "big") % (q - 1) + 1        # noqa: E731
        xs, ks = [rnd() for _ in range(n_keys)], [rnd() for _ in range(n_ops)]
        pw = ctx.modexp_ops(np.repeat(_ints_to_be([g], PB), n_keys + n_ops, axis=0), np.zeros(n_keys + n_ops, dtype=np.uint32), _ints_to_be([p], PB),
                            _ints_to_be(xs + ks, QB))
        keys_y = np.ascontiguousarray(pw[:n_keys])
        assert int.from_bytes(keys_y[0].tobytes(), "big") == pow(g, xs[0], p)
        pq, qq, gq = _ints_to_be([p], PB), _ints_to_be([q], QB), _ints_to_be([g], PB)
        dg = np.frombuffer(rng.bytes(n_ops * dlen), dtype=np.uint8).reshape(n_ops, dlen).copy()
        idx = rng.integers(n_keys, size=n_ops).astype(np.uint32)
        sg_one, sg_many = np.zeros((n_ops, 2 * QB), dtype=np.uint8), np.zeros((n_ops, 2 * QB), dtype=np.uint8)
        for i in range(n_ops):
            r = int.from_bytes(pw[n_keys + i].tobytes(), "big") % q
            z, kinv = int.from_bytes(dg[i].tobytes(), "big"), pow(ks[i], -1, q)
            s1, sm = kinv * (z + r * xs[0]) % q, kinv * (z + r * xs[int(idx[i])]) % q
            assert r and s1 and sm, (name, i)
            rb = r.to_bytes(QB, "big")
            sg_one[i] = np.frombuffer(rb + s1.to_bytes(QB, "big"), dtype=np.uint8)
            sg_many[i] = np.frombuffer(rb + sm.to_bytes(QB, "big"), dtype=np.uint8)
        for sg in (sg_one, sg_many):
            sg[5, 2 * QB - 1] ^= 1                                       # one forgery: the verdicts are not a constant
        valid, stb = np.zeros(n_ops + 8, dtype=np.uint8), np.zeros(n_ops + 8, dtype=np.uint8)

        def checked(rc, count):
            assert rc == 0 and not stb[:count].any(), (name, rc)
            assert valid[:count].sum() == count - (1 if count > 5 else 0) and (count <= 5 or valid[5] == 0), name

        def raw(count, sg, ki, nk):
            t0 = time.perf_counter()
            rc = lib.bftkv_gpu_dsa_verify(h, count, P(dg), dlen, P(sg), QB, P(ki), nk, P(keys_y), None, PB, 1, P(pq), P(qq), P(gq), P(valid), P(stb))
            t = time.perf_counter() - t0
            checked(rc, count)
            return t

        def through_set(handle, count, sg, ki):
            t0 = time.perf_counter()
            rc = lib.bftkv_gpu_dsa_verify_keyset(h, handle, count, P(dg), dlen, P(sg), P(ki), P(valid), P(stb))
            t = time.perf_counter() - t0
            checked(rc, count)
            return t

        def create(nk, w):
            hs = C.c_int(-1)
            t0 = time.perf_counter()
            rc = lib.bftkv_gpu_dsa_keyset_create(h, nk, P(keys_y), None, PB, 1, P(pq), P(qq), P(gq), QB, w, C.byref(hs))
            t = time.perf_counter() - t0
            assert rc in (0, E_NOMEM), (name, w, rc)
            return t, (hs.value if rc == 0 else None)

        shapes = (("one_key", sg_one, None, 1), ("%d_keys" % n_keys, sg_many, idx, n_keys))
        for w in widths:
            row = {"group": name, "window_bits": w, "n": n_ops, "keys": n_keys, "reps": reps}
            # (c) creation, after one warm-up creation (the group's rows and the kernels' code objects)
            warm = create(1, w)[1]
            if warm is None:                     # not even one key's tables fit: nothing of this width is measured
                for k in ("create_1_key", "create_%d_keys" % n_keys, "lone") + tuple(s_[0] for s_ in shapes):
                    row[k] = "not measured"
                print(json.dumps(row), file=sys.stderr, flush=True)
                out.append(row)
                continue
            ctx.dsa_keyset_destroy(warm)
            t_c = {1: [], n_keys: []}
            for _ in range(3):
                for nk in (1, n_keys):
                    t, hs = create(nk, w)
                    if hs is not None:
                        t_c[nk].append(t)
                        ctx.dsa_keyset_destroy(hs)
            row["create_1_key"] = stats(t_c[1]) if t_c[1] else "not measured"
            row["create_%d_keys" % n_keys] = stats(t_c[n_keys]) if t_c[n_keys] else "not measured"
            handles = {1: create(1, w)[1], n_keys: create(n_keys, w)[1]}
            # (a) and (b): warm-up for every shape, then the two entries alternating
            for label, sg, ki, nk in shapes:
                if handles[nk] is None:
                    row[label] = "not measured"
                    continue
                row["table_bytes_" + label] = ctx.dsa_keyset_info(handles[nk])["table_bytes"]
                raw(n_ops, sg, ki, nk)
                through_set(handles[nk], n_ops, sg, ki)
                t_raw, t_set = [], []
                for _ in range(reps):
                    t_raw.append(raw(n_ops, sg, ki, nk))
                    t_set.append(through_set(handles[nk], n_ops, sg, ki))
                r_, s_ = stats(t_raw), stats(t_set)
                row[label] = {"raw": r_, "keyset": s_, "raw_over_keyset": round(r_["median_ms"] / s_["median_ms"], 3),
                              "raw_per_s": round(n_ops / (r_["median_ms"] * 1e-3)), "keyset_per_s": round(n_ops / (s_["median_ms"] * 1e-3)),
                              "faster_beyond_spread": s_["max_ms"] < r_["min_ms"]}
            # (d) a lone verification
            if handles[1] is None:
                row["lone"] = "not measured"
            else:
                raw(1, sg_one, None, 1)
                through_set(handles[1], 1, sg_one, None)
                t_raw, t_set = [], []
                for _ in range(max(reps, 9)):
                    t_raw.append(raw(1, sg_one, None, 1))
                    t_set.append(through_set(handles[1], 1, sg_one, None))
                row["lone"] = {"raw": stats(t_raw), "keyset": stats(t_set)}
            for hs in handles.values():
                if hs is not None:
                    ctx.dsa_keyset_destroy(hs)
            print(json.dumps(row), file=sys.stderr, flush=True)
            out.append(row)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=80000)
    ap.add_argument("--keys", type=int, default=1000)
    ap.add_argument("--groups", default="dsa1024,dsa1536,dsa2048")
    ap.add_argument("--widths", default="4,8,12")
    ap.add_argument("--out")
    a = ap.parse_args()
    res = {"kind": "device", "clock": "host, synchronised C calls; raw entry and key set alternating, %d repetitions each after a warm-up" % a.reps,
           "command": "python tools/dsa_keyset_rate.py --reps %d --n %d --keys %d --groups %s --widths %s" % (a.reps, a.n, a.keys, a.groups, a.widths),
           "runs": run(a.groups.split(","), [int(w) for w in a.widths.split(",")], a.reps, a.n, a.keys)}
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
