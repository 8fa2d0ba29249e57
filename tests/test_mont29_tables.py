"""CPU: the per-key tables of k_rsa_modexp<18,4,29> -- n and (2^2088)^2 mod n as 72 limbs of 29 bits, -n^-1 mod 2^29 -- as
hostbn::mont_setup(.., W = 29) and its defining form mont_setup_by_doubling give them (csrc/host_bignum.h, through
tools/hostcheck/mont_setup_tables.cpp), against Python integers; and the 28-bit tables of the same moduli through the same
program, which must still be what they were."""
import os
import random
import shutil
import subprocess

import pytest

from tests import mont_cases as K28

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _moduli():
    rng = random.Random(7229)
    odd = lambda bits: rng.getrandbits(bits - 1) | (1 << (bits - 1)) | 1          # noqa: E731
    out = [K28.rsa_modulus("full2048"), K28.rsa_modulus("sparse2048"), (1 << 2048) - (1 << 29) - 1, 1, 3, 65537]
    out += [odd(b) for b in (2048, 2047, 1025, 1024, 512, 257, 64, 29, 28)]
    return out


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not on PATH")
    exe = str(tmp_path_factory.mktemp("hostcheck") / "mont_setup_tables")
    subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tools", "hostcheck", "mont_setup_tables.cpp"), "-o", exe],
                   check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    return exe


def _run(tool, W, nl, mods):
    r = subprocess.run([tool, str(W), str(nl)] + ["%x" % n for n in mods], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    lines = r.stdout.decode().split("\n")[:-1]
    assert len(lines) == 2 * len(mods)
    out = []
    for ln in lines:
        f = ln.split()
        v = [int(x, 16) for x in f[2:]]
        assert len(v) == 1 + 2 * nl
        out.append((f[0], int(f[1]), v[0], v[1:1 + nl], v[1 + nl:]))
    return out


def _check(rows, W, nl, mods):
    val = lambda limbs: sum(x << (W * i) for i, x in enumerate(limbs))       # noqa: E731
    for i, n in enumerate(mods):
        for form, ok, n0, nrow, r2 in rows[2 * i:2 * i + 2]:
            assert ok == 1, (form, hex(n))
            assert max(nrow) < 1 << W and max(r2) < 1 << W
            assert val(nrow) == n, (form, hex(n))
            assert val(r2) == pow(2, 2 * W * nl, n), (form, hex(n))
            assert n0 == (-pow(n, -1, 1 << W)) % (1 << W), (form, hex(n))


def test_29_bit_tables_equal_python_integers(tool):
    mods = _moduli()
    _check(_run(tool, 29, 72, mods), 29, 72, mods)


def test_29_bit_tables_next_to_the_limb_capacity(tool):
    """Moduli within two bits of 72 x 29 = 2088 bits are outside mont_setup's contract (R > 4n fails): it hands them to the
    doubling form, and both still give the defining numbers."""
    rng = random.Random(2088)
    mods = [rng.getrandbits(b - 1) | (1 << (b - 1)) | 1 for b in (2086, 2087, 2088)]
    _check(_run(tool, 29, 72, mods), 29, 72, mods)


def test_28_bit_tables_are_what_they_were(tool):
    mods = _moduli()
    _check(_run(tool, 28, 76, mods), 28, 76, mods)
    _check(_run(tool, 28, 80, mods), 28, 80, mods)


def test_even_and_zero_moduli_are_refused(tool):
    for form, ok, *_ in _run(tool, 29, 72, [0, 2, 1 << 2047]):
        assert ok == 0, form
