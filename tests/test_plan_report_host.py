"""plan_report::decide (csrc/plan_report.h) sizes what a resident big verify call enqueues behind its modexp from the words the
device reported.  Compiled for the host with -fsanitize=address,undefined (tests/c/plan_report_host.cpp, a program of its own)
and swept over: words present, absent and inconsistent; packet counts 0, 1, 63, 64, 65, 98,304 and 26.6 M; reported lengths
from 0 to the packet count; rings with and without RSA-3072, RSA-4096 and DSA keys; calls and builds without the pass over
long values, and the main modexp pass on 4 and on 8 lanes per number.  Three properties, restated here in plain Python: every
grid covers whatever could be queued, absent words give the grids over the packet count, to the block, and phase 1's modexp
and inverse grids -- in the queue before any word can arrive -- are those over the packet count in every case."""
import itertools
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from bftkv_amd._native import Context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS = Context.PLAN_REPORT_SLOTS
ARRIVED = 0x80000000
TOTALS = (0, 1, 63, 64, 65, 98304, 26_600_000)
N_HASHES = 7


def ceil_div(a, b):
    return (a + b - 1) // b


def grids_over(total, n_items, ring, wide_form=1, main=64):
    """The grids of a call sized by its packet count alone (run_pipeline without a report)."""
    r3, r4, d2, d3, invb, invs = [(ring >> b) & 1 for b in range(6)]
    dsa = d2 or d3
    g = {"walk_fill": n_items, "mid_other": ceil_div(n_items, 64) * (N_HASHES - 1), "mid_text": ceil_div(n_items, 64) * N_HASHES}
    for ph in ("1", "2"):
        g["wide" + ph] = ceil_div(total, 64) if wide_form else 0
        g["compare" + ph] = ceil_div(total * 4, 256)
        g["compare%s_3072" % ph] = ceil_div(total * 4, 256) if r3 else 0
        g["compare%s_4096" % ph] = ceil_div(total * 4, 256) if r4 else 0
        g["dsa_mul" + ph] = ceil_div(total, 64) if dsa else 0
        g["dsa_split" + ph] = ceil_div(total, 256) if d2 and d3 else 0
        g["dsa_modexp%s_4" % ph] = ceil_div(total, 64) if d2 else 0
        g["dsa_modexp%s_8" % ph] = ceil_div(total, 32) if d3 else 0
    g.update({k[:-1] + "2" + s: v for (k, s), v in phase_1_over(total, ring, main).items()})
    return g


PHASE_1 = (("modexp1", ""), ("modexp1", "_3072"), ("modexp1", "_4096"), ("dsa_inv1", "_batched"), ("dsa_inv1", ""))


def phase_1_over(total, ring, main=64):
    """Phase 1's modexp and inverse grids, which the getter does not report: over the packet count (as phase 2's without a report)."""
    r3, r4, d2, d3, invb, invs = [(ring >> b) & 1 for b in range(6)]
    dsa = d2 or d3
    return dict(zip(PHASE_1, (ceil_div(total, main), ceil_div(total, 32) if r3 else 0, ceil_div(total, 32) if r4 else 0,
                              ceil_div(total, 4096) if dsa and invb else 0, ceil_div(total, 64) if dsa and invs else 0)))


def length_sets(total):
    """(l0, l1, l2, l3) as reported: within the packet count, at its edges, and beyond it."""
    edge = sorted({0, 1, total // 3, total // 2, max(total, 1) - 1, total})
    ok = [t for t in itertools.product(edge, repeat=4) if sum(t) <= total]
    rng = np.random.default_rng(total + 7)
    if len(ok) > 40:
        keep = [(0, 0, 0, 0), (total, 0, 0, 0), (0, total, 0, 0), (0, 0, total, 0), (0, 0, 0, total)]
        ok = keep + [ok[i] for i in rng.choice(len(ok), 35, replace=False)]
    bad = [(total + 1, 0, 0, 0), (0, total + 1, 0, 0), (total, 1, 0, 0), (total // 2 + 1, total // 2 + 1, 0, 0), (0x7FFFFFFF, 0, 0, 0),
           (0, 0, total // 2 + 1, total // 2 + 1)]
    return ok, bad


def make_cases():
    """Per case: the 11 words of the call, its kind, then wide_form and the numbers per block of the main modexp pass."""
    cases = []
    for total in TOTALS:
        n_items = 0 if total == 0 else max(1, total // 53)
        ok, bad = length_sets(total)
        for ring in range(64):
            if (ring & 12) == 0 and (ring & 48):      # inverse kernels without DSA keys: not a call that exists
                continue
            if (ring & 12) and not (ring & 48):       # one of the two inverse kernels is always enqueued
                continue
            # absent: disabled with everything there; enabled with nothing there
            full = [ARRIVED | v for v in ok[-1]]
            cases.append((total, n_items, 0, 1, 0, ARRIVED, *full, ring, "absent"))
            cases.append((total, n_items, 1, 0, 0, 0, 0, 0, 0, 0, ring, "absent"))
            # partly there
            cases.append((total, n_items, 1, 1, 0, ARRIVED, 0, 0, 0, 0, ring, "flags_only"))
            cases.append((total, n_items, 1, 1, 0, ARRIVED | 3, full[0], full[1], 0, full[3], ring, "flags_only"))
            cases.append((total, n_items, 1, 0, 0, 0, *full, ring, "lengths_only"))
            for flags in (0, 1, 2, 3):
                for ln in ok[:: 1 if ring in (0, 63) else 7]:
                    for over in (0, 1, n_items):
                        cases.append((total, n_items, 1, 1, over, ARRIVED | flags, *[ARRIVED | v for v in ln], ring, "present"))
            for ln in bad:
                cases.append((total, n_items, 1, 1, 0, ARRIVED, *[ARRIVED | (v & 0x7FFFFFFF) for v in ln], ring, "inconsistent"))
            cases.append((total, n_items, 1, 1, n_items + 1, ARRIVED, *full, ring, "overflow_inconsistent"))
    cases.append((534164, 10000, 1, 1, 0, ARRIVED, ARRIVED | 439440, ARRIVED, ARRIVED, ARRIVED, 0, "headline"))
    cases = [c + (1, 64) for c in cases]
    # every third call above (the headline apart) again without the pass over long values (a build of the 28-bit form), as the small
    # staged call that puts its main pass on 8 lanes, and -- no call that exists, the geometry alone -- with that pass on 8 lanes
    # beside the long values'
    return cases + [c[:12] + g for g in ((0, 64), (0, 32), (1, 32)) for c in cases[:-1][::3]]


@pytest.fixture(scope="module")
def swept(tmp_path_factory):
    """cases, per case the getter's slots by name, per case phase 1's modexp and inverse grids by PHASE_1"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("plan_report_host")
    exe, fin, fout = str(tmp / "plan_report_host"), str(tmp / "in.bin"), str(tmp / "out.bin")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "c", "plan_report_host.cpp"), "-o", exe], check=True)
    cases = make_cases()
    with open(fin, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            f.write(struct.pack("<13I", *c[:11], *c[12:14]))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, "plan_report_host exited with %d: %s" % (r.returncode, (r.stdout + r.stderr)[-4000:])
    rows = np.fromfile(fout, dtype="<u4").reshape(len(cases), len(SLOTS) + len(PHASE_1))
    return cases, [dict(zip(SLOTS, map(int, row))) for row in rows], [dict(zip(PHASE_1, map(int, row[len(SLOTS):]))) for row in rows]


@pytest.fixture(scope="module")
def decided(swept):
    return swept[:2]


def test_the_sweep_holds_what_it_says(decided):
    cases, _ = decided
    assert {c[0] for c in cases} == set(TOTALS) | {534164}
    assert {c[11] for c in cases} == {"absent", "flags_only", "lengths_only", "present", "inconsistent", "overflow_inconsistent", "headline"}
    assert {c[10] & 15 for c in cases} == set(range(16))
    for total in TOTALS:
        l0 = {c[6] & ~ARRIVED for c in cases if c[0] == total and c[11] == "present"}
        assert {0, total} <= l0
    assert {c[12:14] for c in cases} == {(1, 64), (0, 64), (0, 32), (1, 32)}
    for g in ((0, 64), (0, 32), (1, 32)):
        assert {c[11] for c in cases if c[12:14] == g} >= {"absent", "flags_only", "present", "inconsistent"}
        assert {c[10] & 15 for c in cases if c[12:14] == g} == set(range(16))


def test_absent_words_reproduce_the_grids_over_the_packet_count(decided):
    cases, rows = decided
    n = 0
    for c, d in zip(cases, rows):
        total, n_items, ring, kind = c[0], c[1], c[10], c[11]
        want = grids_over(total, n_items, ring, *c[12:14])
        if kind == "absent":
            assert d["words"] & 7 == 0 and d["phase2_bound"] == total
            assert {k: d[k] for k in want} == want, (c, d)
            n += 1
        elif kind in ("inconsistent", "flags_only"):
            # lengths that cannot be true, or not all there: every length-sized grid as without them
            assert d["words"] & 2 == 0 and d["phase2_bound"] == total, (c, d)
            flags = c[5] & 3
            for k, v in want.items():
                if k in ("wide1", "wide2") and not flags & 2 or k in ("mid_other", "mid_text") and not flags & 1 or k == "walk_fill":
                    continue
                assert d[k] == v, (k, c, d)
            n += 1
        elif kind == "overflow_inconsistent":
            assert d["words"] & 4 == 0 and d["walk_fill"] == n_items
            n += 1
    assert n > 500


def test_every_grid_covers_what_could_be_queued(decided):
    cases, rows = decided
    for c, d in zip(cases, rows):
        total, n_items, enabled, over_arrived, over, flags_word = c[:6]
        ring, kind, wide_form, main = c[10:14]
        r3, r4, d2, d3, invb, invs = [(ring >> b) & 1 for b in range(6)]
        lens_known = kind in ("present", "lengths_only", "overflow_inconsistent", "headline") and enabled
        lens = [w & ~ARRIVED for w in c[6:10]] if lens_known else None
        if lens is not None and ((not r3 and lens[2]) or (not r4 and lens[3]) or (not (d2 or d3) and lens[1])):
            # a list this ring cannot feed is reported non-empty: the words are not this call's, and count as absent
            assert d["words"] & 2 == 0, (c, d)
            lens = None
        assert bool(d["words"] & 2) == (lens is not None), (c, d)
        # what each list can hold in phase 1 and gain in phase 2, at the most
        w1 = lens if lens is not None else [total] * 4
        w2 = total - sum(lens) if lens is not None else total
        assert d["phase2_bound"] == w2
        flags_known = enabled and flags_word & ARRIVED
        wide = bool(wide_form) and (bool(flags_word & 2) if flags_known else True)
        other = bool(flags_word & 1) if flags_known else True
        if wide:
            assert d["wide1"] * 64 >= w1[0] and d["wide2"] * 64 >= w2, (c, d)
        else:
            assert d["wide1"] == 0 and d["wide2"] == 0
        if other:
            assert d["mid_other"] == ceil_div(n_items, 64) * 6 and d["mid_text"] == ceil_div(n_items, 64) * 7
        else:
            assert d["mid_other"] == 0 and d["mid_text"] == 0
        if enabled and over_arrived and over == 0:
            assert d["walk_fill"] == 0
        else:
            assert d["walk_fill"] == n_items      # one block per item
        for ph, work in (("1", w1), ("2", [w2] * 4)):
            assert d["compare" + ph] * 64 >= work[0]
            assert d["compare%s_3072" % ph] * 64 >= (work[2] if r3 else 0)
            assert d["compare%s_4096" % ph] * 64 >= (work[3] if r4 else 0)
            dsa_work = work[1] if (d2 or d3) else 0
            assert d["dsa_mul" + ph] * 64 >= dsa_work
            if d2 and d3:
                assert d["dsa_split" + ph] * 256 >= dsa_work
            else:
                assert d["dsa_split" + ph] == 0
            assert d["dsa_modexp%s_4" % ph] * 64 >= (dsa_work if d2 else 0)
            assert d["dsa_modexp%s_8" % ph] * 32 >= (dsa_work if d3 else 0)
        assert d["modexp2"] * main >= w2
        assert d["modexp2_3072"] * 32 >= (w2 if r3 else 0) and d["modexp2_4096"] * 32 >= (w2 if r4 else 0)
        if d2 or d3:
            assert d["dsa_inv2_batched"] * 4096 >= (w2 if invb else 0) and d["dsa_inv2"] * 64 >= (w2 if invs else 0)
        # ... and no grid is larger than the one over the packet count
        want = grids_over(total, n_items, ring, wide_form, main)
        for k, v in want.items():
            assert d[k] <= v, (k, c, d)
        # what a ring cannot queue is not launched
        if not r3:
            assert d["compare1_3072"] == d["compare2_3072"] == d["modexp2_3072"] == 0
        if not r4:
            assert d["compare1_4096"] == d["compare2_4096"] == d["modexp2_4096"] == 0
        if not (d2 or d3):
            assert all(d[k] == 0 for k in SLOTS if k.startswith("dsa_"))


def test_phase_1_modexp_and_inverses_are_sized_by_the_packet_count(swept):
    """They are in the queue before any word can arrive: ceil(total / per-block) whatever the words say."""
    cases, _, phase1 = swept
    for c, p1 in zip(cases, phase1):
        assert p1 == phase_1_over(c[0], c[10], c[13]), (c, p1)


def test_no_pass_over_long_values_where_the_call_has_none(decided):
    cases, rows = decided
    n = 0
    for c, d in zip(cases, rows):
        if not c[12]:
            assert d["wide1"] == d["wide2"] == 0, (c, d)
            n += 1
    assert n > 1000


def test_the_main_pass_on_eight_lanes_sizes_the_main_grids_alone(swept):
    n = 0
    for c, d, p1 in zip(*swept):
        total, wide_form, main = c[0], c[12], c[13]
        if main != 32:
            continue
        assert p1[PHASE_1[0]] == ceil_div(total, 32) and d["modexp2"] == ceil_div(d["phase2_bound"], 32), (c, d)
        if wide_form and d["wide1"]:      # (the long values stay on 4 lanes: 64 per block, over the list's length / phase 2's bound)
            w1 = (c[6] & ~ARRIVED) if d["words"] & 2 else total
            assert d["wide1"] == ceil_div(w1, 64) and d["wide2"] == ceil_div(d["phase2_bound"], 64), (c, d)
            n += 1
    assert n > 100


def test_the_headline_batch(decided):
    """cfg 2 of the benchmark: 534,164 packets, 439,440 queued in phase 1, SHA-256 only, no long value, no overflow."""
    cases, rows = decided
    (d,) = [d for c, d in zip(cases, rows) if c[11] == "headline"]
    launched = {k: v for k, v in d.items() if v and k not in ("words", "phase2_bound", "total")}
    assert launched == {"compare1": 6867, "modexp2": 1481, "compare2": 1481} and d["phase2_bound"] == 94724 and d["words"] == 15
