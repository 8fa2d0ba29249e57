"""A resident big CollectiveSignature.Verify call sizes what it enqueues behind its modexp by what the device reported about
the batch (csrc/plan_report.h).  The smallest such call -- a 64-replica clique, 1,900 writes, about 100.7 k packets, signed on
the device as bench.py signs -- over: (a) the default mutations, (b) corruption raised until many items need phase 2, (c) one
value s + j n of 262 / 266 bytes in a phase-1 position / only behind an item's phase-1 cut, (d) one SHA-512 signature, (e) one
item that overflows its walk scratch row.  Judged by the C restatement of the reference (oracle/c) on error byte, exit count
and per-packet status (through the count of public-key operations those statuses imply, as bench.py counts them); the
diagnostics getter says what was launched.  (f): every batch again under BFTKV_PLAN_REPORT=0, in a fresh process (the
variable is read once), with identical answers."""
import os
import subprocess
import sys

import numpy as np
import pytest

from bftkv_amd._native import Context
from corpus import build as cb
from tests import helpers as H
from tests import plan_report_cases as K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOT = {k: i for i, k in enumerate(Context.PLAN_REPORT_SLOTS)}


def ceil_div(a, b):
    return (a + b - 1) // b


@pytest.fixture(scope="module")
def world(gpu_ctx, tmp_path_factory):
    from oracle.cbind import COracle
    cl = cb.make_cluster(64)
    mods, exps = cb.signer_tables(cl)
    signer = lambda em, ki: gpu_ctx.modexp(em, ki.astype(np.uint32), mods, exps)
    batches = K.make_batches(cl, signer)
    kr, q = H.oracle_keyring(cl), H.clique_quorum(cl)
    co = COracle()
    co.set_keyring(kr)
    co.set_quorum(q)
    threads = max(1, min(16, os.cpu_count() or 1))
    want = {name: co.collective_verify(*batches[name], n_threads=threads) for name in K.CASES}
    # (b), on the CPU first: the items with two bad values in front are mostly still admitted -- from packets behind the
    # plan's phase-1 cut, so phase 2 has work
    twice = batches["b_twice_bad"]      # (every third item, if unmutated and of at least 45 packets: about 1900 / 3 x 0.5 x 20 / 22 = 288)
    assert len(twice) > 200 and (want["b_corrupt"][0][twice] == 0).mean() > 0.7, (len(twice), (want["b_corrupt"][0][twice] == 0).mean())
    gpu_ctx.keyring_set(H.abi_keys(kr))
    qh = gpu_ctx.quorum_create(H.abi_qcs(q))
    cx = gpu_ctx.fork()
    K.run_resident(cx, qh, batches["a_default"])      # (the fork's first call allocates its arena: not the call to look at)
    got = {}
    for name in K.CASES:
        for _ in range(3):      # (a call whose words all made the host's deadline, if one of three does: _launched)
            got[name] = K.run_resident(cx, qh, batches[name])
            if got[name]["report"][SLOT["words"]] == 15:
                break
    # (f): the same batches under BFTKV_PLAN_REPORT=0, in a fresh process
    tmp = tmp_path_factory.mktemp("plan_report")
    fin, fout = str(tmp / "batches.npz"), str(tmp / "answers.npz")
    K.store_batches(fin, batches)
    env = dict(os.environ, BFTKV_PLAN_REPORT="0")
    r = subprocess.run([sys.executable, "-m", "tests.plan_report_cases", fin, fout], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, (r.stdout + r.stderr)[-4000:])
    z = np.load(fout)
    off = {name: {k: z[name + "." + k] for k in got[name]} for name in K.CASES}
    yield {"cl": cl, "batches": batches, "want": want, "got": got, "off": off}
    cx.close()
    gpu_ctx.quorum_destroy(qh)


def _judge(world, name, g):
    import bench
    cerr, cnver, ops = world["want"][name]
    n = len(cerr)
    assert (g["err"] == cerr).all() and (g["nver"] == cnver).all(), (name, np.flatnonzero(g["err"] != cerr)[:10], np.flatnonzero(g["nver"] != cnver)[:10])
    assert bench.reference_pubkey_ops(g["st"], g["st_item"], g["err"], g["nver"], n) == ops, name
    return g["report"]


def _launched(rep, wide=False, other=False, overflow=False):
    """What the getter must say for an RSA-2048 ring, given what the batch holds and WHICH words the call had in hand: a word
    that missed the host's deadline is no failure -- that call gets the grids over the packet count (the fixture asks up to
    three times for a call that had them all, and the host sweep covers the sizing itself)."""
    words, total, bound = int(rep[SLOT["words"]]), int(rep[SLOT["total"]]), int(rep[SLOT["phase2_bound"]])
    assert words & 8 and total >= K.MIN_PACKETS
    if not words & 1:
        wide = other = True
    if not words & 4:
        overflow = True
    if words & 2:
        assert 0 < bound < total
    else:
        assert bound == total
    queued1 = total - bound if words & 2 else total
    want = {"walk_fill": K.N_ITEMS if overflow else 0,
            "mid_other": ceil_div(K.N_ITEMS, 64) * 6 if other else 0, "mid_text": ceil_div(K.N_ITEMS, 64) * 7 if other else 0,
            "wide1": ceil_div(queued1, 64) if wide else 0, "wide2": ceil_div(bound, 64) if wide else 0,
            "compare1": ceil_div(queued1, 64), "modexp2": ceil_div(bound, 64), "compare2": ceil_div(bound, 64)}
    for k in ("compare1_3072", "compare1_4096", "modexp2_3072", "modexp2_4096", "dsa_mul1", "dsa_mul2", "dsa_inv2", "dsa_inv2_batched"):
        want[k] = 0
    assert {k: int(rep[SLOT[k]]) for k in want} == want, words
    return words, total, bound


def test_a_default_mutations(world):
    rep = _judge(world, "a_default", world["got"]["a_default"])
    _launched(rep)


def test_b_many_items_need_phase_2(world):
    g = world["got"]["b_corrupt"]
    rep = _judge(world, "b_corrupt", g)
    words, total, bound = _launched(rep)
    # Phase 1 cuts an item at 44 clique members; with two bad values in front that leaves 42 good ones, one short: an item of
    # these that is admitted (most are: the fixture's check, and _judge holds the device to the oracle) was admitted by phase 2.
    twice = world["batches"]["b_twice_bad"]
    assert (g["err"][twice] == 0).mean() > 0.7
    if words & 2:      # ... and with the lengths in hand, counted: each such item queues what lies behind its cut, 1 to 20 packets
        assert int(g["pubkey_ops"][0]) - (total - bound) > len(twice)


@pytest.mark.parametrize("name", ["c_wide_phase1", "c_wide_phase2"])
def test_c_a_value_too_long_for_the_29_bit_form(world, name):
    g = world["got"][name]
    rep = _judge(world, name, g)
    _launched(rep, wide=True)
    item = int(world["batches"]["items"][0 if name == "c_wide_phase1" else 1])
    mine = np.flatnonzero(g["st_item"] == item)
    pos = mine[1] if name == "c_wide_phase1" else mine[-1]
    assert g["st"][pos] == 0 and g["err"][item] == 0         # the long value verified (ST_OK), in whichever phase reached it


def test_d_one_sha512_signature(world):
    g = world["got"]["d_sha512"]
    rep = _judge(world, "d_sha512", g)
    _launched(rep, other=True)
    item = int(world["batches"]["items"][2])
    assert g["st"][np.flatnonzero(g["st_item"] == item)[3]] == 0


def test_e_one_item_overflows_its_scratch_row(world):
    g = world["got"]["e_overflow"]
    rep = _judge(world, "e_overflow", g)
    _launched(rep, overflow=True)
    assert (g["st_item"] == int(world["batches"]["items"][3])).sum() > 700


@pytest.mark.parametrize("name", K.CASES)
def test_f_the_same_answers_without_the_report(world, name):
    on, off = world["got"][name], world["off"][name]
    for k in ("err", "nver", "verdict", "fenced", "st", "st_item", "pubkey_ops"):
        assert (on[k] == off[k]).all(), (name, k)
    rep = off["report"]
    total = int(rep[SLOT["total"]])
    assert rep[SLOT["words"]] == 0 and rep[SLOT["phase2_bound"]] == total
    assert rep[SLOT["walk_fill"]] == K.N_ITEMS and rep[SLOT["mid_other"]] and rep[SLOT["mid_text"]]
    for k in ("wide1", "wide2", "modexp2", "compare1", "compare2"):
        assert rep[SLOT[k]] == ceil_div(total, 64), k
