"""-m gpu: the field and point arithmetic of csrc/ec_field.h on the device, operation by operation, on the raw word rows of
tests/ec_form_cases.py -- Montgomery-form words at and around 0, m, R mod m and every word boundary, all ordered pairs of them
through fe_mul, fe_add and fe_sub with every class of the last conditional subtraction, carries out of the top word and borrows
through every word; points of smallest and largest x under Z = 1, Z = p - 1, random and extremal Z; infinity with X and Y left in
place; equal and opposite points under different Z in every aliasing form of pt_add and pt_add_affine; scalars at and above the
order in pt_mul; every window of fb_mul's walk -- against exact integer expectations, which tests/test_ec_forms_reference.py holds
to the same operation table compiled for the CPU and to tests/ec_ref.py.  The limb conversions of ec_kernels.hip, which exist on
the device only, are checked here alone.

tests/c/ec_forms.hip is compiled here (not by build(): it is no part of the library) and run ONCE, as a child process under a
time limit, on one input file: per curve and operation family the whole set shuffled, so that neighbouring lanes hold different
cases and a lane that leaves pt_add early sits beside one that does not, then the head of that list cut at 1, 63, 64, 65 and 129
records, the wave and block ends.  A non-zero exit or a timeout fails the module's fixture: every test then errors and nothing
starts the program again.

Observed: as one command (hipcc --offload-arch=gfx950 -O3, 52 kernels that inline the ladder, the inversion and the table walk on
up to 17 words) the program cross-compiles without warnings in 127 s on a build host without a GPU, 66 s of it the 17-word
kernels.  This module therefore compiles one object per curve and main side by side (-DEC_FORMS_ONLY_L) and links them: 14.9 s
on an MI355X host.  The run takes 1.28 s there (312 launches, some 149,000 records, most of it the runtime's start and the copies);
the comparison with the exact answers takes about 2 s per session."""
import os
import shutil
import subprocess
import time

import pytest

import ec_form_cases as F
import ec_ref as E

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN_LIMIT_S = 60          # the kernels take well under a second; a minute means it hangs
_ATTEMPTED = []           # the driver is started at most once per session, whatever became of it
GROUPS = {"field": (F.FAM_FE, F.FAM_INV, F.FAM_FN), "addition": (F.FAM_DBL, F.FAM_ADD, F.FAM_ADDA), "ladder": (F.FAM_MUL,), "table walk": (F.FAM_FB,),
          "in and out": (F.FAM_AFF, F.FAM_CHK, F.FAM_H2I, F.FAM_XR), "limbs": (F.FAM_LIMBS,)}
FAMS = tuple(range(len(F.FAM_NAMES)))
assert sorted(fam for g in GROUPS.values() for fam in g) == list(FAMS)


def _compile(tmp):
    """One object per curve and one for main, side by side (tests/c/ec_forms.hip, EC_FORMS_ONLY_L), then the link."""
    src = os.path.join(ROOT, "tests", "c", "ec_forms.hip")
    base = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wall", "-Werror"]
    objs = [str(tmp / ("ec_forms_%d.o" % part)) for part in (0, 7, 8, 12, 17)]
    procs = [subprocess.Popen(base + ["-DEC_FORMS_ONLY_L=%d" % part, "-c", src, "-o", obj], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for part, obj in zip((0, 7, 8, 12, 17), objs)]
    outs = [p.communicate()[0] for p in procs]
    for p, out in zip(procs, outs):
        assert p.returncode == 0, out[-4000:]
    exe = str(tmp / "ec_forms")
    r = subprocess.run(base + objs + ["-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.fixture(scope="module")
def device_rows(tmp_path_factory):
    """{(curve, family): [per section [row bytes]]} from one run of the driver."""
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    assert not _ATTEMPTED, "the driver has been started once and did not finish cleanly; it is not started again"
    tmp = tmp_path_factory.mktemp("ec_forms")
    fin, fout = str(tmp / "in.bin"), str(tmp / "out.bin")
    t0 = time.time()
    exe = _compile(tmp)
    t_compile = time.time() - t0
    with open(fin, "wb") as f:
        for name in E.NAMES:
            f.write(F.curve_block(name))
        for name in E.NAMES:
            for fam in FAMS:
                for sec in F.sections(name, fam):
                    f.write(F.pack(name, fam, sec))
    _ATTEMPTED.append(exe)
    t0 = time.time()
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=RUN_LIMIT_S)      # TimeoutExpired kills the child and fails the fixture
    t_run = time.time() - t0
    print("ec_forms: compiled in %.1f s, ran in %.2f s: %s" % (t_compile, t_run, r.stdout.strip()))
    assert r.returncode == 0, "ec_forms exited with %d: %s" % (r.returncode, (r.stdout + r.stderr)[-2000:])
    buf = open(fout, "rb").read()
    out, off = {}, 0
    for name in E.NAMES:
        for fam in FAMS:
            out[(name, fam)] = []
            for sec in F.sections(name, fam):
                got, off = F.rows(name, fam, len(sec), buf, off)
                out[(name, fam)].append(got)
    assert off == len(buf)
    return out


def _compare(name, fam, sec, got):
    cs = F.cases(name, fam)
    assert len(got) == len(sec)
    bad = [(pos, cs[i].label, what) for pos, (i, row) in enumerate(zip(sec, got)) for what in [F.check(name, fam, cs[i], row)] if what]
    assert not bad, "%s %s: %d of %d records differ from the exact answer (position, case, rows): %s" % (name, F.FAM_NAMES[fam], len(bad), len(sec), bad[:8])


@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("name", E.NAMES)
def test_whole_set_shuffled_and_cut_at_wave_and_block_ends(device_rows, name, group):
    """Per family the whole set in one launch, then 1, 63, 64, 65 and 129 records: what follows the last one is an idle lane, or
    nothing."""
    for fam in GROUPS[group]:
        secs = F.sections(name, fam)
        assert [len(s) for s in secs[1:]] == list(F.CUTS) and len(secs[0]) == len(F.cases(name, fam))
        for sec, got in zip(secs, device_rows[(name, fam)]):
            _compare(name, fam, sec, got)


@pytest.mark.parametrize("name", E.NAMES)
def test_neighbouring_lanes_hold_different_cases(device_rows, name):
    """In the shuffled pt_add section most waves hold all four case codes: a lane that leaves early sits beside one that does not."""
    cs = F.cases(name, F.FAM_ADD)
    sec = F.sections(name, F.FAM_ADD)[0]
    waves = [sec[j:j + 64] for j in range(0, len(sec) - 63, 64)]
    assert len(waves) >= 5 and sum(len({cs[i].tag for i in w}) == 4 for w in waves) >= len(waves) - 1
    codes = [int.from_bytes(row[-4:], "little") for row in device_rows[(name, F.FAM_ADD)][0]]
    assert codes == [cs[i].tag for i in sec]
