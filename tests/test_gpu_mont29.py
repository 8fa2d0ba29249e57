"""-m gpu: the 18 x 4 form of the Montgomery multiplier at radix 2^29 (csrc/mont28.h with W = 29, the form of
k_rsa_modexp<18,4,29>) on the operand set of tests/mont29_cases.py against the lane-by-lane model at 29 bits, which
tests/test_mont29_model.py holds to exact integer arithmetic: the lazy output limb for limb, the rows after canonicalize and
after reduce_once as limbs and as integers.

tests/c/mont_form29.hip is compiled here and run ONCE, as a child process under a time limit, on one input file: the whole
set shuffled, so that neighbouring groups hold different moduli and operations, then the head of that list cut so that the
last working group sits at and just past the end of a DPP row, a wave and a block.  A non-zero exit or a timeout fails the
module's fixture: every test then errors and nothing starts the program again."""
import os
import shutil
import subprocess
import time

import pytest

from tests import mont29_cases as K
from tests import mont_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN_LIMIT_S = 60          # the run takes well under a second; a minute means it hangs
_ATTEMPTED = []           # the driver is started at most once per session, whatever became of it


def _sections():
    order = K.shuffled()
    return [order] + [order[:g] for g in K.cut_sizes()]


@pytest.fixture(scope="module")
def device_rows(tmp_path_factory):
    """[per section [(lazy, canonical, reduced)]] from one run of the driver."""
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    assert not _ATTEMPTED, "the driver has been started once and did not finish cleanly; it is not started again"
    tmp = tmp_path_factory.mktemp("mont_form29")
    exe, fin, fout = str(tmp / "mont_form29"), str(tmp / "in.bin"), str(tmp / "out.bin")
    t0 = time.time()
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", os.path.join(ROOT, "tests", "c", "mont_form29.hip"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    t_compile = time.time() - t0
    cs = K.cases()
    with open(fin, "wb") as f:
        for sec in _sections():
            f.write(K.pack([cs[i] for i in sec]))
    _ATTEMPTED.append(exe)
    t0 = time.time()
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=RUN_LIMIT_S)      # TimeoutExpired kills the child and fails the fixture
    print("mont_form29: compiled in %.1f s, ran in %.2f s: %s" % (t_compile, time.time() - t0, r.stdout.strip()))
    assert r.returncode == 0, "mont_form29 exited with %d: %s" % (r.returncode, (r.stdout + r.stderr)[-2000:])
    buf = open(fout, "rb").read()
    out, off = [], 0
    for sec in _sections():
        rows, off = K.unpack(len(sec), buf, off)
        out.append(rows)
    assert off == len(buf)
    return out


def _compare(sec, got):
    cs, (exp, _) = K.cases(), K.expected()
    bad = []
    for pos, (i, (lazy, canon, red)) in enumerate(zip(sec, got)):
        e_lazy, e_canon, e_red = exp[i]
        what = [name for name, g, e in (("lazy", lazy, e_lazy), ("canonical", canon, e_canon), ("reduced", red, e_red)) if g != e]
        if K.from_limbs(canon) != K.from_limbs(lazy) or K.from_limbs(red) != cs[i].residue:
            what.append("value")
        if what:
            bad.append((pos, cs[i].label, what))
    assert not bad, "%d of %d groups differ from the model (position, case, rows): %s" % (len(bad), len(sec), bad[:8])


def test_whole_set_shuffled(device_rows):
    sec = _sections()[0]
    cs = K.cases()
    per_row = M.ROW // K.TPI
    assert len(sec) == len(cs) > 256 // K.TPI                                      # more than one block
    assert sum(len({cs[i].nval for i in sec[j:j + per_row]}) > 1 for j in range(0, len(sec), per_row)) > len(sec) // per_row // 2
    _compare(sec, device_rows[0])


def test_last_group_at_row_wave_and_block_ends(device_rows):
    """1, 4, 5, 16, 17, 64 and 65 groups: what follows the last one is padding that repeats it, or nothing."""
    secs = _sections()
    assert [len(s) for s in secs[1:]] == K.cut_sizes() == [1, 4, 5, 16, 17, 64, 65]
    for sec, got in zip(secs[1:], device_rows[1:]):
        _compare(sec, got)
