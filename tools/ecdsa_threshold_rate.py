"""Threshold-ECDSA rates on the device: per curve, 10,000 CalculateR operations at k = 8 (the reference's n = 10, 2t = 8) and
k = 22 (64 nodes), a lone call, and the ec_scalar_base_mult rate, for both work splits (BFTKV_EC_SPLIT: 1 = a lane per term
and an ordered fold, 2 = a lane per operation; P-521 has only the first).  Times are a synchronised host clock around whole
calls (median of --reps); field products per operation are counted from the algorithm (ec_field.h).

    python tools/ecdsa_threshold_rate.py [--reps 3] [--out rate.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAC_ROOF = 29.66e12      # 32x32->64 multiply-adds per second, profiles/r02_valu_issue_rates_microbench.txt


def field_products(bits: int, k: int) -> int:
    """Per CalculateR operation: per term 5 + 2 (Unmarshal's check, l w mod N), 8 per doubling and 16 per addition of the
    left-to-right multiplication (half the bits set); the fold's k - 1 additions and one Fermat inversion (bits squarings and
    about bits / 2 products) with the affine x."""
    term = 7 + 8 * bits + 16 * (bits // 2)
    return k * term + 16 * (k - 1) + bits + bits // 2 + 5


def child(split: int, reps: int):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import ec_ref as E
    from bftkv_amd import Context
    ctx = Context(0)
    out = []
    rng = np.random.default_rng(1)
    for name in E.NAMES:
        c = E.CURVES[name]
        n, bits = c["n"], c["bit_size"]
        if split == 2 and bits > 384:
            continue
        words = (bits + 31) // 32
        scal = [int.from_bytes(rng.bytes(80), "big") % n for _ in range(10000 * 8)]
        t0 = time.perf_counter()
        pts, st = ctx.ec_scalar_base_mult(scal, c)
        t_bm = time.perf_counter() - t0
        assert not st.any()
        rec = {"curve": name, "split": "term" if split == 1 else "op", "base_mult_80k_ms": round(t_bm * 1e3, 2)}
        for k in (8, 22):
            n_ops = 10000
            xs = [list(range(1, k + 1))] * n_ops
            ri = [pts[(i * k) % (len(pts) - k):(i * k) % (len(pts) - k) + k] for i in range(n_ops)]
            vi = [[scal[(i + j) % len(scal)] for j in range(k)] for i in range(n_ops)]
            ctx.ecdsa_calculate_r(xs[:64], ri[:64], vi[:64], c)            # warm-up
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                _, st = ctx.ecdsa_calculate_r(xs, ri, vi, c)
                ts.append(time.perf_counter() - t0)
            lone = []
            for _ in range(reps):
                t0 = time.perf_counter()
                ctx.ecdsa_calculate_r(xs[:1], ri[:1], vi[:1], c)
                lone.append(time.perf_counter() - t0)
            ms = sorted(ts)[len(ts) // 2] * 1e3
            fp = field_products(bits, k)
            rec["k%d" % k] = {"ms_10k": round(ms, 2), "ms_lone": round(sorted(lone)[len(lone) // 2] * 1e3, 3),
                              "field_products_per_op": fp,
                              "mac_rate_of_roof": round(fp * 2 * words * words * n_ops / (ms * 1e-3) / MAC_ROOF, 4)}
        out.append(rec)
    ctx.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--child", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reps)
        return
    res = {"kind": "device", "clock": "host, synchronised calls", "runs": []}
    for split in (1, 2):
        env = dict(os.environ, BFTKV_EC_SPLIT=str(split))
        p = subprocess.run([sys.executable, __file__, "--child", str(split), "--reps", str(a.reps)], env=env, capture_output=True, text=True,
                           timeout=600)
        if p.returncode != 0:
            res["runs"].append({"split": split, "error": p.stderr[-2000:]})
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
