"""CPU: the EC operation table (tests/c/ec_forms.h, the text tests/c/ec_forms.hip runs on the device) compiled by g++ over every case
of tests/ec_form_cases.py but the limb conversions, against the exact expectations; the conditions that make that set worth
running (every class of fe_mul's last step, every pt_add case code in every aliasing form, the exceptional additions inside the
ladder and the table walk); and the module's own group law and hash integer against tests/ec_ref.py and tests/ecdsa_verify_ref.py
on a sample, so that the new Python does not grade itself."""
import collections
import ctypes as C
import os
import random
import subprocess

import pytest

import ec_form_cases as F
import ec_ref as E
import ecdsa_verify_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAM_IDS = [F.FAM_NAMES[fam] for fam in F.HOST_FAMS]


@pytest.fixture(scope="module")
def efh(tmp_path_factory):
    so = tmp_path_factory.mktemp("ec_forms_host") / "ec_forms_host.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                    os.path.join(ROOT, "tests", "c", "ec_forms_host.cpp"), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.efh_run.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_char_p, C.c_char_p]
    lib.efh_run.restype = C.c_int
    return lib


def host_rows(lib, name, fam, idx):
    cx = F.ctx(name)
    cs = F.cases(name, fam)
    cb = b"".join(cx.c[k].to_bytes(cx.f, "big") for k in ("p", "n", "b", "gx", "gy"))
    out = C.create_string_buffer(4 * F.out_words(cx.L, fam) * len(idx))
    assert lib.efh_run(cb, cx.f, cx.bits, fam, len(idx), b"".join(cs[i].rec for i in idx), out) == 0
    return F.rows(name, fam, len(idx), out.raw, 0)[0]


@pytest.mark.parametrize("fam", F.HOST_FAMS, ids=FAM_IDS)
@pytest.mark.parametrize("name", E.NAMES)
def test_host_compiled_table_against_the_expectations(efh, name, fam):
    cs = F.cases(name, fam)
    idx = F.order(name, fam)
    assert sorted(idx) == list(range(len(cs)))
    got = host_rows(efh, name, fam, idx)
    bad = [(pos, cs[i].label, what) for pos, (i, row) in enumerate(zip(idx, got)) for what in [F.check(name, fam, cs[i], row)] if what]
    assert not bad, "%d of %d records differ (position, case, what): %s" % (len(bad), len(idx), bad[:8])


def test_limbs_are_the_device_programs_alone(efh):
    cx = F.ctx("P-256")
    assert efh.efh_run(b"\0" * (5 * cx.f), cx.f, cx.bits, F.FAM_LIMBS, 0, b"", C.create_string_buffer(4)) == -1
    for name in E.NAMES:
        assert len(F.cases(name, F.FAM_LIMBS)) > 64


@pytest.mark.parametrize("name", E.NAMES)
def test_fe_mul_classes(name):
    """At least 10 cases in each class of the value t before fe_mul's last subtraction, under p and under n: t < m, m <= t < 2^(32 L)
    and t >= 2^(32 L).  The third cannot occur on P-521: both moduli are below 2^521, so t < 2 m < 2^(32 L) = 2^544."""
    cx = F.ctx(name)
    count = collections.Counter(cs.tag[1:] for cs in F.cases(name, F.FAM_FE) if cs.tag[0] == "mul" and cs.label.startswith("fe_mul %s: " % "pn"[cs.tag[1]]))
    print(name, sorted(count.items()))
    for mod, m in enumerate((cx.p, cx.n)):
        assert count[(mod, 0)] >= 10 and count[(mod, 1)] >= 10, (name, mod)
        if name == "P-521":
            assert 2 * m < cx.R and count[(mod, 2)] == 0
        else:
            assert 2 * m > cx.R and count[(mod, 2)] >= 10, (name, mod)
    # the model that classifies is a Montgomery product: t = a b / R mod m, below 2 m
    rng = random.Random(1)
    for mod, m in enumerate((cx.p, cx.n)):
        for _ in range(20):
            a, b = rng.randrange(m), rng.randrange(m)
            t = F.cios_t(a, b, m, cx.L)
            assert t < 2 * m and t % m == a * b * pow(cx.R, -1, m) % m


@pytest.mark.parametrize("name", E.NAMES)
def test_carries_and_borrows_are_present(name):
    cx = F.ctx(name)
    fe = F.cases(name, F.FAM_FE)
    for mod, m in enumerate((cx.p, cx.n)):
        carry = sum(cs.tag == ("add", mod, True) for cs in fe)
        assert (carry >= 8) if 2 * (m - 1) >= cx.R else (carry == 0), (name, mod, carry)           # the full-width moduli only
        assert sum(cs.tag == ("sub", mod, True) for cs in fe) >= 100 and sum(cs.tag == ("sub", mod, False) for cs in fe) >= 100
    xr = collections.Counter(cs.tag for cs in F.cases(name, F.FAM_XR))
    assert xr["x = r"] >= 2 and xr["x = r + n"] >= 2 and xr["r + n >= p"] >= 2, xr
    assert (xr["carry"] >= 6) if 2 * cx.n - 1 >= cx.R else (xr["carry"] == 0), xr
    verdicts = collections.Counter(cs.exp for cs in F.cases(name, F.FAM_XR))
    assert min(verdicts.values()) >= 10 and len(verdicts) == 2
    if name in ("P-384", "P-521"):                    # x = p - 1 is on the curve: alpha = 0 in pt_dbl
        assert any(pt[0] == cx.p - 1 for _, pt in F.special_x_points(name))
    if name != "P-224":
        assert F.special_x_points(name)[0][1][0] == 0


@pytest.mark.parametrize("name", E.NAMES)
def test_every_case_code_in_every_form(name):
    for fam, forms in ((F.FAM_ADD, ("R distinct", "R is P", "R is Q")), (F.FAM_ADDA, ("R distinct", "R is P"))):
        seen = collections.Counter((cs.label.split(":")[0].split(", ")[1], cs.tag) for cs in F.cases(name, fam))
        for form in forms:
            for code in (F.GENERAL, F.EQUAL, F.OPPOSITE, F.INF_OPERAND):
                assert seen[(form, code)] >= 4, (name, F.FAM_NAMES[fam], form, F.CODE_NAMES[code], seen[(form, code)])
    labels = [cs.label for cs in F.cases(name, F.FAM_ADD)]
    for what in ("P + P, equal Z", "P + P, different Z", "P + (-P), equal Z", "P + (-P), different Z", "infinity, Z = 0 under G's X, Y + infinity"):
        assert any(what in lab for lab in labels), (name, what)


@pytest.mark.parametrize("name", E.NAMES)
def test_exceptional_additions_inside_the_ladder_and_the_walk(name):
    """The labelled scalars meet what their labels say, by the exact group law: k = n ends on OPPOSITE, k = n + 2 on EQUAL, k = 2 n + 1
    (which fits in L words on P-521 only) on INF_OPERAND; on P-521 the walk of one k >= n meets EQUAL in the top window."""
    cx = F.ctx(name)
    want = {F.OPPOSITE, F.EQUAL} | ({F.INF_OPERAND} if name == "P-521" else set())
    met = set()
    for cs in F.cases(name, F.FAM_MUL):
        last, P, k = cs.tag
        if last is not None:
            assert F.CODE_NAMES[last] in cs.label
            if P == cx.g:
                codes = F.ladder_codes(cx, P, k)
                # (2 n + 1 passes n - 1 and n on its way: OPPOSITE, then the addition to infinity)
                mid = codes[1:-2] + [F.GENERAL] if last == F.INF_OPERAND and codes[-2] == F.OPPOSITE else codes[1:-1]
                assert codes[0] == F.INF_OPERAND and codes[-1] == last and all(c == F.GENERAL for c in mid), (name, cs.label)
            met.add(last)
        if k >= cx.n:
            met.add("k >= n")
    assert met == want | {"k >= n"}, (name, met)
    top = [cs for cs in F.cases(name, F.FAM_FB) if cs.tag[0] is not None]
    assert len(top) == (len(F.FB_W) if name == "P-521" else 0)
    for cs in top:
        meet, w, nwin, k = cs.tag
        codes = F.walk_codes(cx, w, nwin, k)
        assert k >= cx.n and codes[-1] == meet and codes[0][1] == F.INF_OPERAND and all(c == F.GENERAL for _, c in codes[1:-1]), (name, cs.label)
    for t, w in enumerate(F.FB_W):
        nwin = F.fb_windows(cx, w)
        labels = {cs.label for cs in F.cases(name, F.FAM_FB)}
        assert all(f"fb_mul w = {w}: one digit, window {i}" in labels for i in range(nwin - 1)), (name, w)


@pytest.mark.parametrize("name", E.NAMES)
def test_expectations_agree_with_the_restatement_on_a_sample(name):
    """The affine group law of ec_form_cases.py against ec_ref.py's Jacobian restatement of Go's code, on the very expectations of a
    seeded sample of cases; its hash integer against ecdsa_verify_ref.py's."""
    cx, c = F.ctx(name), E.CURVES[name]
    rng = random.Random(3)
    aff = lambda P: (0, 0) if P is None else P      # noqa: E731
    for cs in rng.sample(F.cases(name, F.FAM_DBL), 10):
        J = F.ints(cx, cs.rec, 3)
        got = E.affine_from_jacobian(c, *E.double_jacobian(c, *(cx.from_m(v) for v in J)))
        assert got == aff(cs.exp), (name, cs.label)
    sample = rng.sample(F.cases(name, F.FAM_ADD), 30)
    assert len({cs.tag for cs in sample}) >= 3
    for cs in sample:
        J = [cx.from_m(v) for v in F.ints(cx, cs.rec, 6, off=1)]
        got = E.affine_from_jacobian(c, *E.add_jacobian(c, *J))
        assert got == aff(cs.exp[0]), (name, cs.label)
    for cs in rng.sample(F.cases(name, F.FAM_MUL), 12) + rng.sample(F.cases(name, F.FAM_FB), 12):
        _, P, k = cs.tag[:3] if cs.label.startswith("pt_mul") else (None, cx.g, cs.tag[3])
        if P is not None:
            assert E.scalar_mult(c, P[0], P[1], E.int_bytes(k)) == aff(cs.exp), (name, cs.label)
    for cs in F.cases(name, F.FAM_H2I):
        d = cs.rec[4:4 + cs.tag]
        assert int.from_bytes(cs.exp, "little") == V.hash_to_int(c, d) % c["n"], (name, cs.label)
    for cs in rng.sample(F.cases(name, F.FAM_XR), 12):
        J = F.ints(cx, cs.rec, 4)
        x, _ = E.affine_from_jacobian(c, *(cx.from_m(v) for v in J[:3]))
        assert cs.exp == F.u32(int(x % cx.n == J[3])), (name, cs.label)


def test_the_device_programs_sections():
    """The shuffled whole, then its head at 1, 63, 64, 65 and 129 records; lists shorter than a cut go round again."""
    for name in E.NAMES:
        for fam in range(len(F.FAM_NAMES)):
            secs = F.sections(name, fam)
            n = len(F.cases(name, fam))
            assert [len(s) for s in secs] == [n, 1, 63, 64, 65, 129] and n <= 1 << 16
            assert all(s == [secs[0][i % n] for i in range(len(s))] for s in secs[1:])
            assert len(F.pack(name, fam, secs[2])) == 12 + 63 * 4 * F.in_words(F.WORDS[name], fam)
