"""-m gpu: the four forms of the library's Montgomery multiplier (csrc/mont28.h: <19,4>, <10,8>, <14,8> on the ring window,
<19,8> on the window that normalises at block boundaries) on the operand set of tests/mont_cases.py -- full and sparse
moduli, limbs of 2^28, operands up to 2n - 1, x = R - 1, chains of lazy outputs, outputs at and just above n -- against the
lane-by-lane model (tests/mont_model.py), which tests/test_mont_model.py holds to exact integer arithmetic.  The lazy output is
compared limb for limb, the rows after canonicalize and after reduce_once as limbs and as integers.

tests/c/mont_forms.hip is compiled here (not by build(): it is no part of the library) and run ONCE, as a child process under
a time limit, on one input file: per form the whole set shuffled, so that the groups beside each other hold different moduli
and operations, then the head of that list cut so that the last working group sits at and just past the end of a DPP row, a
wave and a block.  A non-zero exit or a timeout fails the module's fixture: every test then errors and nothing starts the
program again.

Observed on an MI355X host: the compile takes 3.2 s, the run 0.30 s (32 launches, about 2,900 groups, most of it the runtime's
start); the model's side of the comparison takes 1 to 4 s per form, once per session."""
import os
import shutil
import subprocess
import time

import pytest

from tests import mont_cases as K
from tests import mont_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORM_IDS = [K.form_id(f) for f in K.FORMS]
RUN_LIMIT_S = 60          # the run takes 0.3 s (a few seconds where the runtime starts cold); a minute means it hangs
_ATTEMPTED = []           # the driver is started at most once per session, whatever became of it


def _sections(form):
    """[(indices into cases(form))]: the shuffled whole, then its head at each cut size."""
    order = K.shuffled(form)
    return [order] + [order[:g] for g in K.cut_sizes(form)]


@pytest.fixture(scope="module")
def device_rows(tmp_path_factory):
    """{form: [per section [(lazy, canonical, reduced)]]} from one run of the driver."""
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    assert not _ATTEMPTED, "the driver has been started once and did not finish cleanly; it is not started again"
    tmp = tmp_path_factory.mktemp("mont_forms")
    exe, fin, fout = str(tmp / "mont_forms"), str(tmp / "in.bin"), str(tmp / "out.bin")
    t0 = time.time()
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", os.path.join(ROOT, "tests", "c", "mont_forms.hip"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    t_compile = time.time() - t0
    with open(fin, "wb") as f:
        for form in K.FORMS:
            cs = K.cases(form)
            for sec in _sections(form):
                f.write(K.pack(form, [cs[i] for i in sec]))
    _ATTEMPTED.append(exe)
    t0 = time.time()
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=RUN_LIMIT_S)      # TimeoutExpired kills the child and fails the fixture
    t_run = time.time() - t0
    print("mont_forms: compiled in %.1f s, ran in %.2f s: %s" % (t_compile, t_run, r.stdout.strip()))
    assert r.returncode == 0, "mont_forms exited with %d: %s" % (r.returncode, (r.stdout + r.stderr)[-2000:])
    buf = open(fout, "rb").read()
    out, off = {}, 0
    for form in K.FORMS:
        out[form] = []
        for sec in _sections(form):
            rows, off = K.unpack(form, len(sec), buf, off)
            out[form].append(rows)
    assert off == len(buf)
    return out


def _compare(form, sec, got):
    cs, (exp, _) = K.cases(form), K.expected(form)
    bad = []
    for pos, (i, (lazy, canon, red)) in enumerate(zip(sec, got)):
        e_lazy, e_canon, e_red = exp[i]
        what = [name for name, g, e in (("lazy", lazy, e_lazy), ("canonical", canon, e_canon), ("reduced", red, e_red)) if g != e]
        if M.from_limbs(canon) != M.from_limbs(lazy) or M.from_limbs(red) != cs[i].residue:
            what.append("value")
        if what:
            bad.append((pos, cs[i].label, what))
    assert not bad, "%d of %d groups differ from the model (position, case, rows): %s" % (len(bad), len(sec), bad[:8])


@pytest.mark.parametrize("form", K.FORMS, ids=FORM_IDS)
def test_whole_set_shuffled(device_rows, form):
    sec = _sections(form)[0]
    cs = K.cases(form)
    per_row = M.ROW // form[1]
    assert len(sec) == len(cs) > 256 // form[1]                                    # more than one block
    assert sum(len({cs[i].nval for i in sec[j:j + per_row]}) > 1 for j in range(0, len(sec), per_row)) > len(sec) // per_row // 2
    _compare(form, sec, device_rows[form][0])


@pytest.mark.parametrize("form", K.FORMS, ids=FORM_IDS)
def test_last_group_at_row_wave_and_block_ends(device_rows, form):
    """1, 16/TPI, 16/TPI + 1, 64/TPI, 64/TPI + 1, 256/TPI and 256/TPI + 1 groups: what follows the last one is padding that
    repeats it, or nothing."""
    secs = _sections(form)
    assert [len(s) for s in secs[1:]] == K.cut_sizes(form)
    for sec, got in zip(secs[1:], device_rows[form][1:]):
        _compare(form, sec, got)
