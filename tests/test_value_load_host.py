"""value_limbs (csrc/value_load.h), the branch-free loader of a signature value's limbs, compiled for the host with
-fsanitize=address,undefined (tests/c/value_load_host.cpp, a program of its own) and run over heap buffers of exactly nb bytes:
every nb from 0 to 540, all five lane forms, random / all-FF / all-00 / one-bit contents, against plain integer slicing.  A read
outside [value, value + nb) ends the program with a sanitizer report."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import value_load_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_rows(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("value_load_host")
    exe, fin, fout = str(tmp / "value_load_host"), str(tmp / "in.bin"), str(tmp / "out.bin")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "c", "value_load_host.cpp"), "-o", exe], check=True)
    rng = np.random.default_rng(20261019)
    values = [v for nb in range(541) for v in K.contents(nb, rng)]
    with open(fin, "wb") as f:
        f.write(struct.pack("<I", len(values)))
        for v in values:
            f.write(struct.pack("<I", len(v)) + v)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, "value_load_host exited with %d: %s" % (r.returncode, (r.stdout + r.stderr)[-4000:])
    per_value = sum(L * TPI for L, TPI, _ in K.FORMS)
    rows = np.fromfile(fout, dtype="<u4")
    assert rows.size == len(values) * per_value
    return values, rows.reshape(len(values), per_value)


def test_every_length_and_content(host_rows):
    values, rows = host_rows
    assert len(values) == 3 + 540 * 5 and {len(v) for v in values} == set(range(541))
    bad = []
    for v, row in zip(values, rows.tolist()):
        off = 0
        for L, TPI, W in K.FORMS:
            if row[off:off + L * TPI] != K.limbs(v, L, TPI, W):
                bad.append((len(v), v[:2].hex(), (L, TPI, W)))
            off += L * TPI
    assert not bad, "%d (value, form) pairs differ from integer slicing (nb, first bytes, form): %s" % (len(bad), bad[:8])


def test_lengths_reach_past_every_form():
    """540 bytes are more than the widest form holds (19 x 8 x 28 bits = 532 bytes), and one set bit lands in its top limb."""
    assert max(L * TPI * W for L, TPI, W in K.FORMS) == 532 * 8 < 540 * 8
    top = K.limbs(b"\x80" + b"\x00" * 531, 19, 8, 28)
    assert top[-1] == 1 << 27 and not any(top[:-1])
