"""-m gpu: value_limbs (csrc/value_load.h) behind a bare kernel, k_value_load<L,TPI,W>, in the lane geometry of k_rsa_modexp and
with its memory functors, for all five forms, against plain integer slicing.

Values of 0 ... 532 bytes lie inside one blob at every start alignment 0 ... 15, each between guard bytes of A5: a dword fetched from
a wrong offset shows as a wrong limb (under an all-zero value: as any non-zero limb), not as a fault.  tests/c/value_load.hip is
compiled here and run ONCE, as a child process under a time limit, on one input file: per form the whole set shuffled, then its
head cut so that the last working group sits at and just past the end of a DPP row, a wave and a block.  A non-zero exit or a
timeout fails the module's fixture: every test then errors and nothing starts the program again."""
import os
import random
import shutil
import struct
import subprocess
import time

import numpy as np
import pytest

from tests import value_load_cases as K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN_LIMIT_S = 60          # the run takes well under a second; a minute means it hangs
_ATTEMPTED = []           # the driver is started at most once per session, whatever became of it

NBS = [0, 1, 3, 4, 5, 8, 64, 65, 66, 67, 130, 131, 255, 256, 257, 261, 262, 266, 384, 385, 512, 513, 532]
CUTS = [1, 4, 5, 16, 17, 64, 65]
GUARD = 0xA5


def _cases():
    """(nb, alignment, bytes): random contents at every (nb, alignment), all-zero ones once per nb; shuffled."""
    rng = np.random.default_rng(9)
    cs = [(nb, al, rng.bytes(nb)) for nb in NBS for al in range(16)] + [(nb, nb % 16, b"\x00" * nb) for nb in NBS]
    random.Random(9).shuffle(cs)
    return cs


def _blob(cs):
    """[(offset, nb)] and the blob: 16 ... 31 guard bytes before each value, so that it starts at its alignment, and 16 behind the last."""
    blob, recs = bytearray(), []
    for nb, al, v in cs:
        blob += bytes([GUARD]) * 16
        blob += bytes([GUARD]) * ((al - len(blob)) % 16)
        assert len(blob) % 16 == al
        recs.append((len(blob), nb))
        blob += v
    blob += bytes([GUARD]) * 16
    return recs, bytes(blob)


def _sections():
    cs = _cases()
    return [(form, sec) for form in K.FORMS for sec in [cs] + [cs[:g] for g in CUTS]]


@pytest.fixture(scope="module")
def device_rows(tmp_path_factory):
    """[per section [limbs per value]] from one run of the driver."""
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    assert not _ATTEMPTED, "the driver has been started once and did not finish cleanly; it is not started again"
    tmp = tmp_path_factory.mktemp("value_load")
    exe, fin, fout = str(tmp / "value_load"), str(tmp / "in.bin"), str(tmp / "out.bin")
    t0 = time.time()
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", os.path.join(ROOT, "tests", "c", "value_load.hip"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    t_compile = time.time() - t0
    with open(fin, "wb") as f:
        for (L, TPI, W), sec in _sections():
            recs, blob = _blob(sec)
            f.write(struct.pack("<5I", L, TPI, W, len(sec), len(blob)))
            f.write(b"".join(struct.pack("<2I", o, nb) for o, nb in recs))
            f.write(blob)
    _ATTEMPTED.append(exe)
    t0 = time.time()
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=RUN_LIMIT_S)      # TimeoutExpired kills the child and fails the fixture
    print("value_load: compiled in %.1f s, ran in %.2f s: %s" % (t_compile, time.time() - t0, r.stdout.strip()))
    assert r.returncode == 0, "value_load exited with %d: %s" % (r.returncode, (r.stdout + r.stderr)[-2000:])
    buf = np.fromfile(fout, dtype="<u4")
    out, off = [], 0
    for (L, TPI, W), sec in _sections():
        n = len(sec) * L * TPI
        out.append(buf[off:off + n].reshape(len(sec), L * TPI).tolist())
        off += n
    assert off == buf.size
    return out


def _compare(form, sec, got):
    L, TPI, W = form
    bad = [(pos, nb, al) for pos, ((nb, al, v), row) in enumerate(zip(sec, got)) if row != K.limbs(v, L, TPI, W)]
    assert not bad, "<%d,%d,%d>: %d of %d values differ from integer slicing (position, nb, alignment): %s" % (L, TPI, W, len(bad), len(sec), bad[:8])


@pytest.mark.parametrize("form", K.FORMS, ids=lambda f: "%dx%dx%d" % f)
def test_every_length_and_alignment(device_rows, form):
    cs = _cases()
    assert {(nb, al) for nb, al, _ in cs} == {(nb, al) for nb in NBS for al in range(16)} and len(cs) > 256 // 4   # more than one block
    hit = [got for (f, sec), got in zip(_sections(), device_rows) if f == form and len(sec) == len(cs)]
    assert len(hit) == 1
    _compare(form, cs, hit[0])


@pytest.mark.parametrize("form", K.FORMS, ids=lambda f: "%dx%dx%d" % f)
def test_last_group_at_row_wave_and_block_ends(device_rows, form):
    """1, 4, 5, 16, 17, 64 and 65 groups: what follows the last one is padding that repeats it, or nothing."""
    cs = _cases()
    hit = [(sec, got) for (f, sec), got in zip(_sections(), device_rows) if f == form and len(sec) < len(cs)]
    assert [len(sec) for sec, _ in hit] == CUTS
    for sec, got in hit:
        _compare(form, sec, got)
