"""tests/c/ecdsa_keyset_host.cpp (the key-set pieces of ec_field.h compiled for the CPU) behind ctypes, for the CPU and the GPU
key-set tests.  Not collected.

    lib = build(directory)                       g++, as tests/test_ecdsa_verify_reference.py compiles its host pieces
    h = Host(lib, curve)
    h.table(w, base)  -> uint32 words            fb_table_build; base = (x, y), or None for the overload that takes G itself
    h.mul(w, base, k) -> (x, y)                  fb_mul over that table
    h.verify(w, key, sig, digest) -> (valid, status)    the kernels' chain with the key's table
    chosen_scalars(c, w, rng)                    the scalars at which a table walk can go wrong"""
import ctypes as C
import os
import subprocess

import numpy as np

import ec_ref as E
import ecdsa_verify_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = {"P-224": 7, "P-256": 8, "P-384": 12, "P-521": 17}


def build(directory):
    so = os.path.join(str(directory), "ecdsa_keyset_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                    os.path.join(ROOT, "tests", "c", "ecdsa_keyset_host.cpp"), "-o", so], check=True)
    lib = C.CDLL(so)
    lib.ekh_table.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_void_p, C.c_uint64]
    lib.ekh_mul.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_char_p, C.c_char_p]
    lib.ekh_verify.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_char_p]
    for fn in (lib.ekh_table, lib.ekh_mul, lib.ekh_verify):
        fn.restype = C.c_int
    return lib


def windows(c, w):
    return (8 * E.byte_len(c) + w - 1) // w


def table_words(c, w):
    """fb_table_words: windows x 2 L x 2^w"""
    return (windows(c, w) * 2 * ((8 * E.byte_len(c) + 31) // 32)) << w


def rnd(rng, c):
    return int.from_bytes(rng.bytes(E.byte_len(c) + 8), "big") % c["n"]


def chosen_scalars(c, w, rng):
    """The scalars at which a table walk can go wrong: 1, N - 1, a lone digit in the first, a middle and the last non-empty
    window (on P-521 the last one holds one bit), every digit 2^w - 1, every other digit zero, and 50 random ones."""
    n, bits = c["n"], c["n"].bit_length()
    last = (bits - 1) // w
    digits = lambda f: sum(f(i) << (w * i) for i in range(last + 1))      # noqa: E731
    ks = [1, n - 1, 1, 1 << (w * (last // 2)), 1 << (w * last)]
    ks += [digits(lambda i: (1 << w) - 1) % n, digits(lambda i: ((1 << w) - 1) * (i & 1)) % n, digits(lambda i: 1 + (i % ((1 << w) - 1)) * (~i & 1)) % n]
    ks += [rnd(rng, c) or 1 for _ in range(50)]
    assert all(0 < k < n for k in ks)
    return ks


class Host:
    def __init__(self, lib, c):
        self.lib, self.c, self.f = lib, c, E.byte_len(c)
        self.L = (8 * self.f + 31) // 32
        self.cb = b"".join(c[k].to_bytes(self.f, "big") for k in ("p", "n", "b", "gx", "gy"))

    def _base(self, base):
        return None if base is None else base[0].to_bytes(self.f, "big") + base[1].to_bytes(self.f, "big")

    def table(self, w, base):
        words = np.zeros(table_words(self.c, w), dtype=np.uint32)
        assert self.lib.ekh_table(self.cb, self.f, w, self._base(base), words.ctypes.data, len(words)) == 0
        return words

    def entry(self, words, w, i, j):
        """Entry j of window i of a table, out of Montgomery form: (x, y)."""
        L, p = self.L, self.c["p"]
        rinv = pow(1 << (32 * L), -1, p)
        at = lambda k: int(words[((i * 2 * L + k) << w) + j])                              # noqa: E731
        x = sum(at(k) << (32 * k) for k in range(L))
        y = sum(at(L + k) << (32 * k) for k in range(L))
        assert x < p and y < p                    # fully reduced: the form is unique
        return x * rinv % p, y * rinv % p

    def mul(self, w, base, k):
        out = C.create_string_buffer(2 * self.f)
        assert self.lib.ekh_mul(self.cb, self.f, w, self._base(base), k.to_bytes(self.f, "big"), out) == 0
        return int.from_bytes(out.raw[:self.f], "big"), int.from_bytes(out.raw[self.f:], "big")

    def verify(self, w, key, sig, digest):
        n = self.c["n"]
        _, s = V.split_sig(self.c, sig)
        winv = pow(s, -1, n) if 0 < s < n else 1
        out = C.create_string_buffer(2)
        assert self.lib.ekh_verify(self.cb, self.f, self.c["bit_size"], w, key, sig, winv.to_bytes(self.f, "big"), digest, len(digest), out) == 0
        return out.raw[0], out.raw[1]
