"""RSA-verification rates on the device: SHA-256 signatures under RSA-2048 keys through bftkv_gpu_rsa_verify_dev and
bftkv_gpu_rsa_verify_keyset_dev, timed with events on the context's stream (arrays resident, after a warm-up call), alternating with
the yardstick in the same process: Context.modexp over the same values with e as exponent bytes plus the host-side EM compare, the
only way to do this job before these entries existed (host clock: it brings 256 bytes per signature back).  Median / min / max of
--reps; every verdict of every call is checked.

Keys: 1, 64, or one per signature.  The first 64 are keys of tests/golden/keys_rsa2048.json with honest signatures (every 7th
mutated); "one per signature" pads the table with further distinct odd 2048-bit moduli that nobody can sign under -- their random
signatures must all come back invalid -- which costs the device the same work and exposes the host's serial mont_setup and the row
upload.

    python tools/rsa_verify_rate.py [--reps 5] [--sizes 1000,10000,100000,430000] [--keys 1,64,n] [--out profiles/rsa_verify_rate.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(ts[len(ts) // 2] * 1e3, 3), "min_ms": round(ts[0] * 1e3, 3), "max_ms": round(ts[-1] * 1e3, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1000,10000,100000,430000")
    ap.add_argument("--keys", default="1,64,n")
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch
    import rsa_verify_ref as V
    from bftkv_amd import Context
    from bftkv_amd._native import _ints_to_be
    ctx = Context(0)
    lib, h = ctx.lib, ctx.h
    stream = torch.cuda.ExternalStream(int(lib.bftkv_gpu_stream(h)))
    P = lambda x: x.ctypes.data_as(C.c_void_p)        # noqa: E731
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")    # noqa: E731
    rng = np.random.default_rng(1)
    raw = json.load(open(os.path.join(ROOT, "tests", "golden", "keys_rsa2048.json")))["keys"][:64]
    real = [(int(k["p"], 16), int(k["q"], 16), int(k["e"], 16)) for k in raw]
    E = real[0][2]
    assert all(e == E for _, _, e in real)
    # a pool of honest signatures per real key (signing is host work outside every clock)
    POOL = 4
    pool = []
    for p, q, e in real:
        n, d = p * q, pow(e, -1, (p - 1) * (q - 1))
        row = []
        for _ in range(POOL):
            dg = rng.bytes(32)
            row.append((dg, pow(int.from_bytes(V.em(256, 8, dg), "big"), d, n).to_bytes(256, "big")))
        pool.append(row)
    runs = []
    for n_ops in [int(v) for v in a.sizes.split(",")]:
        for kspec in a.keys.split(","):
            n_keys = n_ops if kspec == "n" else int(kspec)
            if n_keys > n_ops:
                continue
            n_real = min(n_keys, len(real))
            mods = [p * q for p, q, _ in real[:n_real]]
            base = mods[0]
            mods += [(base ^ (j << 1)) | (1 << 2047) | 1 for j in range(1, n_keys - n_real + 1)]          # distinct, odd, 2048 bits
            key_idx = (np.arange(n_ops) % n_keys).astype(np.uint32)
            dgs, sgs, expect = [], [], np.zeros(n_ops, dtype=np.uint8)
            junk = rng.bytes(256)
            for i in range(n_ops):
                ki = int(key_idx[i])
                if ki < n_real:
                    dg, sg = pool[ki][(i // n_keys) % POOL]
                    if i % 7 == 3:
                        sg = sg[:-1] + bytes([sg[-1] ^ 1])
                    else:
                        expect[i] = 1
                else:
                    dg, sg = pool[0][0][0], junk
                dgs.append(dg); sgs.append(sg)
            dg = np.frombuffer(b"".join(dgs), dtype=np.uint8).copy()
            sg = np.frombuffer(b"".join(sgs), dtype=np.uint8).copy()
            kn = _ints_to_be(mods, 256)
            ke = np.full(n_keys, E, dtype=np.uint32)
            em = np.frombuffer(b"".join(V.em(256, 8, d) for d in dgs), dtype=np.uint8).reshape(n_ops, 256)
            d_dg, d_sg, d_ki = up(dg), up(sg), up(key_idx.view(np.int32))
            d_valid = torch.zeros(n_ops, dtype=torch.uint8, device="cuda:0")
            d_st = torch.zeros(n_ops, dtype=torch.uint8, device="cuda:0")

            def checked():
                ctx.sync()
                assert (d_valid.cpu().numpy() == expect).all() and not bool(d_st.any())
                d_valid.fill_(0x55)

            def timed(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                w0 = time.perf_counter()
                e0.record(stream)
                rc = fn()
                e1.record(stream)
                e1.synchronize()
                w = time.perf_counter() - w0
                assert rc == 0
                checked()
                return e0.elapsed_time(e1) * 1e-3, w

            def raw_call():
                return lib.bftkv_gpu_rsa_verify_dev(h, n_ops, d_dg.data_ptr(), 8, 32, d_sg.data_ptr(), 256, d_ki.data_ptr(), n_keys, P(kn), P(ke),
                                                    d_valid.data_ptr(), d_st.data_ptr())

            t0 = time.perf_counter()
            ks = ctx.rsa_keyset_create(list(zip(mods, [E] * n_keys)), nbytes=256) if n_keys <= (1 << 20) else None
            t_create = time.perf_counter() - t0

            def set_call():
                return lib.bftkv_gpu_rsa_verify_keyset_dev(h, ks, n_ops, d_dg.data_ptr(), 8, 32, d_sg.data_ptr(), d_ki.data_ptr(), d_valid.data_ptr(),
                                                           d_st.data_ptr())

            sg2, eb = sg.reshape(n_ops, 256), _ints_to_be([E] * n_keys, 4)

            def yardstick():
                w0 = time.perf_counter()
                out = ctx.modexp(sg2, key_idx, kn, eb)
                ok = (out == em).all(axis=1).astype(np.uint8)
                w = time.perf_counter() - w0
                assert (ok == expect).all()
                return w

            timed(raw_call); yardstick()                                  # warm-up: rows into the caches, scratch allocated
            if ks is not None:
                timed(set_call)
            t_raw, w_raw, t_set, w_set, t_yard = [], [], [], [], []
            for _ in range(a.reps):                                       # alternating
                t, w = timed(raw_call); t_raw.append(t); w_raw.append(w)
                if ks is not None:
                    t, w = timed(set_call); t_set.append(t); w_set.append(w)
                t_yard.append(yardstick())
            row = {"n_ops": n_ops, "n_keys": n_keys, "raw_events": stats(t_raw), "raw_wall": stats(w_raw), "yardstick_wall": stats(t_yard),
                   "keyset_create_ms": round(t_create * 1e3, 2)}
            if ks is not None:
                row.update(keyset_events=stats(t_set), keyset_wall=stats(w_set))
                ctx.rsa_keyset_destroy(ks)
            row["raw_us_per_sig"] = round(row["raw_events"]["median_ms"] * 1e3 / n_ops, 4)
            runs.append(row)
            print(json.dumps(row), flush=True)
    ctx.close()
    res = {"kind": "device", "what": "SHA-256 under RSA-2048, e = %d" % E,
           "clock": "events on the context's stream around the _dev entries (wall: host clock around the same call incl. the wait); yardstick: host "
                    "clock around Context.modexp + the EM compare; %d alternating repetitions" % a.reps, "runs": runs}
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
