"""Batches for tests/test_gpu_plan_report.py: the smallest resident big call (a 64-replica clique, 1,900 signed writes, about
100.7 k signature packets; the path starts at 98,304) and what is patched into it, plus the one routine that runs a batch
through the resident entry point and collects everything the tests compare.  Run as a program it is the child process of
case (f): it loads the batches its parent stored, runs each under the environment it was given, and stores the answers."""
import sys

import numpy as np

from corpus import build as cb
from tests import rsa_sizes as RS

N_ITEMS = 1900
PKT = 287                       # a DetachSign packet under an RSA-2048 key
MIN_PACKETS = 98304             # TURNSTILE_MIN_PACKETS (csrc/capi.hip)
RAISED = {cb.MUT_BAD_MPI: 0.30, cb.MUT_UNKNOWN_ISSUER: 0.05, cb.MUT_DUP_SIGNER: 0.10, cb.MUT_ONE_SHORT: 0.05}
CASES = ("a_default", "b_corrupt", "c_wide_phase1", "c_wide_phase2", "d_sha512", "e_overflow")


def streams(c):
    return [c.ss_blob[int(c.ss_off[i]):int(c.ss_off[i + 1])].tobytes() for i in range(c.n_items)]


def cat(parts):
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64)
    return np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), off


def signer_of(cl, pkt):
    """the replica whose key id stands in the issuer subpacket of a DetachSign packet"""
    body = pkt[3:] if pkt[1] >= 192 else pkt[2:]
    assert body[12:14] == b"\x09\x10"
    kid = int.from_bytes(body[14:22], "big")
    (kp,) = [r for r in cl.replicas if r.key_id == kid]
    return kp


def rsa_packet(kp, tbss, hash_id=8, nbytes=None):
    """A valid signature packet by kp over tbss; nbytes: the value as s + j n of that many bytes."""
    k = (kp.n.bit_length() + 7) // 8
    prefix, digest = RS.digest_of(kp, tbss, hash_id)
    s = kp.rsa_private(int.from_bytes(RS.encode(k, dict(RS.HASHES)[hash_id], digest), "big"))
    if nbytes is None:
        return RS.packet(prefix, digest, RS.go_mpi(s, k))
    v = s + ((1 << (8 * nbytes)) - 1 - s) // kp.n * kp.n
    assert v % kp.n == s and v >> (8 * nbytes - 8) != 0
    return RS.packet(prefix, digest, RS.go_mpi(v, nbytes))


def flip_value(pkt):
    b = bytearray(pkt)
    b[-5] ^= 0x10
    return bytes(b)


def clean_item(c, cl, min_packets, skip=()):
    for i in range(c.n_items):
        if i not in skip and c.mutation[i] == cb.MUT_NONE and int(c.sig_count[i]) >= min_packets:
            return i
    raise AssertionError("no such item")


def make_batches(cl, signer):
    """name -> (tbs_blob, tbs_off, ss_blob, ss_off)"""
    base = cb.make_write_corpus(cl, N_ITEMS, seed=cb.MASTER_SEED + 10, batch_signer=signer, with_client_sig=True)
    assert base.n_sigs >= MIN_PACKETS, base.n_sigs
    ss = streams(base)
    out = {"a_default": (base.tbss_blob, base.tbss_off, base.ss_blob, base.ss_off)}

    def patched(patch):
        s2 = list(ss)
        for i, data in patch.items():
            s2[i] = data
        sb, so = cat(s2)
        return base.tbss_blob, base.tbss_off, sb, so

    # (b) corruption raised, and in every third untouched item two bad values among the first three packets: more than the
    # plan's margin of one absorbs, with packets left for phase 2
    raised = cb.make_write_corpus(cl, N_ITEMS, seed=cb.MASTER_SEED + 11, batch_signer=signer, with_client_sig=True, mutation_rates=RAISED)
    rs = streams(raised)
    twice = [i for i in range(raised.n_items) if raised.mutation[i] == cb.MUT_NONE and i % 3 == 0 and int(raised.sig_count[i]) >= cl.suff + 2]
    for i in twice:
        p = [rs[i][j:j + PKT] for j in range(0, len(rs[i]), PKT)]
        p[0], p[2] = flip_value(p[0]), flip_value(p[2])
        rs[i] = b"".join(p)
    sb, so = cat(rs)
    assert raised.n_sigs >= MIN_PACKETS, raised.n_sigs
    out["b_corrupt"] = (raised.tbss_blob, raised.tbss_off, sb, so)
    out["b_twice_bad"] = np.array(twice, dtype=np.int64)

    # (c) one value s + j n of 262 bytes in a phase-1 position; one of 266 bytes only behind an item's phase-1 cut, in an item
    # that needs phase 2 (two bad values in front)
    i1 = clean_item(base, cl, cl.suff + 4)
    p = [ss[i1][j:j + PKT] for j in range(0, len(ss[i1]), PKT)]
    p[1] = rsa_packet(signer_of(cl, p[1]), base.tbss(i1), nbytes=262)
    out["c_wide_phase1"] = patched({i1: b"".join(p)})
    i2 = clean_item(base, cl, cl.suff + 5, skip=(i1,))
    p = [ss[i2][j:j + PKT] for j in range(0, len(ss[i2]), PKT)]
    p[0], p[1] = flip_value(p[0]), flip_value(p[1])
    p[-1] = rsa_packet(signer_of(cl, p[-1]), base.tbss(i2), nbytes=266)
    out["c_wide_phase2"] = patched({i2: b"".join(p)})

    # (d) one SHA-512 signature in a SHA-256 batch
    i3 = clean_item(base, cl, cl.suff + 2, skip=(i1, i2))
    p = [ss[i3][j:j + PKT] for j in range(0, len(ss[i3]), PKT)]
    p[3] = rsa_packet(signer_of(cl, p[3]), base.tbss(i3), hash_id=10)
    out["d_sha512"] = patched({i3: b"".join(p)})

    # (e) one item with more packet events than any walk scratch row holds (the row is capped at 320)
    i4 = clean_item(base, cl, cl.suff + 2, skip=(i1, i2, i3))
    out["e_overflow"] = patched({i4: ss[i4][:3 * PKT] + (cb._hdr(13, 1) + b"x") * 700 + ss[i4][3 * PKT:]})
    out["items"] = np.array([i1, i2, i3, i4], dtype=np.int64)
    return out


def run_resident(ctx, qh, batch, report=True):
    """One bftkv_gpu_collective_verify_dev call over device-resident inputs; everything a test compares, as numpy arrays.
    report=False: a call below the big path, which the plan-report getter does not describe."""
    import torch
    tb, to, sb, so = batch
    n = len(to) - 1
    dev = torch.device("cuda:0")
    pad = np.zeros(64, dtype=np.uint8)
    d_tb = torch.from_numpy(np.concatenate([tb, pad])).to(dev)
    d_sb = torch.from_numpy(np.concatenate([sb, pad])).to(dev)
    d_to = torch.from_numpy(np.ascontiguousarray(to, dtype=np.uint64).view(np.int64)).to(dev)
    d_so = torch.from_numpy(np.ascontiguousarray(so, dtype=np.uint64).view(np.int64)).to(dev)
    err = torch.zeros(n, dtype=torch.uint8, device=dev)
    nver = torch.zeros(n, dtype=torch.int32, device=dev)
    verdict = torch.zeros(n, dtype=torch.uint8, device=dev)
    fenced = torch.zeros(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.collective_verify_dev(qh, n, d_tb.data_ptr(), d_to.data_ptr(), d_sb.data_ptr(), d_so.data_ptr(), int(so[-1]),
                              err.data_ptr(), nver.data_ptr(), verdict.data_ptr(), fenced.data_ptr())
    ctx.sync()
    st, st_item = ctx.last_statuses()
    rep = ctx.last_plan_report() if report else dict.fromkeys(ctx.PLAN_REPORT_SLOTS, 0)
    ops = ctx.last_counters()["pubkey_ops"]
    return {"err": err.cpu().numpy(), "nver": nver.cpu().numpy().astype(np.uint32), "verdict": verdict.cpu().numpy(),
            "fenced": fenced.cpu().numpy(), "st": st.copy(), "st_item": st_item.copy(),
            "report": np.array([rep[k] for k in ctx.PLAN_REPORT_SLOTS], dtype=np.uint32), "pubkey_ops": np.array([ops], dtype=np.uint64)}


def store_batches(path, batches):
    flat = {}
    for name in CASES:
        for k, a in zip(("tb", "to", "sb", "so"), batches[name]):
            flat[name + "." + k] = a
    np.savez(path, **flat)


def load_batches(path):
    z = np.load(path)
    return {name: tuple(z[name + "." + k] for k in ("tb", "to", "sb", "so")) for name in CASES}


def main(argv):
    """child of case (f): <batches.npz> <answers.npz>, under the environment of its parent's choosing"""
    import torch  # noqa: F401  (its HIP runtime first: see tests/conftest.py)
    from bftkv_amd import Context
    from tests import helpers as H
    batches = load_batches(argv[1])
    cl = cb.make_cluster(64)
    ctx = Context(0)
    ctx.keyring_set(H.abi_keys(H.oracle_keyring(cl)))
    qh = ctx.quorum_create(H.abi_qcs(H.clique_quorum(cl)))
    flat = {}
    run_resident(ctx, qh, batches[CASES[0]])      # (the first call allocates the arena)
    for name in CASES:
        for k, a in run_resident(ctx, qh, batches[name]).items():
            flat[name + "." + k] = a
    np.savez(argv[2], **flat)
    ctx.close()
    return 0


if __name__ == "__main__":      # python -m tests.plan_report_cases, from the repository root
    sys.exit(main(sys.argv))
