"""tests/c/dsa_keyset_host.cpp (the key-set pieces of dsa_verify.h compiled for the CPU) behind ctypes, and the Python model of a
resident DSA key set, for the CPU and the GPU key-set tests.  Not collected.

    lib = build(directory)                        g++, as tests/ecdsa_keyset_host.py compiles its host pieces
    h = Host(lib)
    h.windows(qbits, w), h.digit(limbs10, window, w), h.entry(base, window, d, windows, w), h.limbs10(exponent)
    h.prep(sig, qbytes, q, digest) -> (status, decided, u1 limbs, u2 limbs, r limbs)
    table(b, p, w, windows) -> [windows][2^w - 1] ints      b^(d 2^(w i)) mod p by pow(), out of Montgomery form
    table_words(b, p, w, windows) -> uint32 [windows][2^w - 1][76]      the same as the device stores it (times R = 2^2128, reduced)
    Model(h, groups, keys, w, qbytes).verify(digest, sig, key) -> (valid, status)       the kernels' chain over lazy pow() tables"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMBS, R = 76, 1 << 2128


def build(directory):
    so = os.path.join(str(directory), "dsa_keyset_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                    os.path.join(ROOT, "tests", "c", "dsa_keyset_host.cpp"), "-o", so], check=True)
    lib = C.CDLL(so)
    u32 = C.c_uint32
    lib.dkh_prep.argtypes = [C.c_char_p, u32, C.c_char_p, C.c_char_p, u32, C.c_char_p, C.c_void_p]
    lib.dkh_prep.restype = C.c_int
    lib.dkh_limbs10.argtypes = [C.c_char_p, u32, C.c_void_p]
    lib.dkh_limbs10.restype = C.c_int
    lib.dkh_windows.argtypes = [u32, u32]
    lib.dkh_windows.restype = u32
    lib.dkh_digit.argtypes = [C.c_void_p, u32, u32]
    lib.dkh_digit.restype = u32
    lib.dkh_entry.argtypes = [u32, u32, u32, u32, u32]
    lib.dkh_entry.restype = C.c_uint64
    lib.dkh_entry_limbs.argtypes = []
    lib.dkh_entry_limbs.restype = u32
    return lib


class Host:
    def __init__(self, lib):
        self.lib = lib
        assert lib.dkh_entry_limbs() == LIMBS

    def windows(self, qbits, w):
        return int(self.lib.dkh_windows(qbits, w))

    def digit(self, limbs10, window, w):
        return int(self.lib.dkh_digit(limbs10.ctypes.data, window, w))

    def digits(self, limbs10, windows, w):
        return [self.digit(limbs10, i, w) for i in range(windows)]

    def entry(self, base, window, d, windows, w):
        return int(self.lib.dkh_entry(base, window, d, windows, w))

    def limbs10(self, e: int):
        out = np.zeros(10, dtype=np.uint32)
        assert self.lib.dkh_limbs10(e.to_bytes(32, "big"), 32, out.ctypes.data) == 0
        return out

    def prep(self, sig: bytes, qbytes: int, q: int, digest: bytes):
        flags, limbs = C.create_string_buffer(2), np.zeros(30, dtype=np.uint32)
        assert self.lib.dkh_prep(sig, qbytes, q.to_bytes(qbytes, "big"), digest, len(digest), flags, limbs.ctypes.data) == 0
        return flags.raw[0], flags.raw[1], limbs[:10].copy(), limbs[10:20].copy(), limbs[20:].copy()


@functools.lru_cache(maxsize=64)
def window_bases(b: int, p: int, w: int, windows: int):
    """B_i = b^(2^(w i)) mod p"""
    out = [b % p]
    for _ in range(windows - 1):
        out.append(pow(out[-1], 1 << w, p))
    return tuple(out)


def table(b: int, p: int, w: int, windows: int):
    return [[pow(B, d, p) for d in range(1, 1 << w)] for B in window_bases(b, p, w, windows)]


def table_words(b: int, p: int, w: int, windows: int) -> np.ndarray:
    """The table as the device holds it: every entry times R mod p, in [0, p), as 76 limbs of 28 bits."""
    out = np.zeros((windows, (1 << w) - 1, LIMBS), dtype=np.uint32)
    for i, row in enumerate(table(b, p, w, windows)):
        for j, v in enumerate(row):
            m = v * R % p
            out[i, j] = [(m >> (28 * k)) & 0xFFFFFFF for k in range(LIMBS)]
    return out


def decode(words) -> int:
    return sum(int(v) << (28 * k) for k, v in enumerate(words))


class Model:
    """A key set as the device holds it -- the groups' g first, then the keys' y, one table per base indexed by the header's own
    entry function -- with entries computed by pow() when the chain first touches them."""

    def __init__(self, h: Host, groups, keys, w: int, qbytes: int):
        self.h, self.groups, self.w, self.qbytes = h, groups, w, qbytes
        self.keys = [(min(g, len(groups) - 1), y) for g, y in keys]
        self.windows = h.windows(max(max(q.bit_length() for _, q, _ in groups), 1), w)
        self.nent = (1 << w) - 1
        self.touched = set()

    def _entry(self, index: int) -> int:
        """What lies at `index` of tab[base][window][d - 1]"""
        d1, rest = index % self.nent, index // self.nent
        window, base = rest % self.windows, rest // self.windows
        n_groups = len(self.groups)
        if base < n_groups:
            b, p = self.groups[base][2], self.groups[base][0]
        else:
            grp, b = self.keys[base - n_groups]
            p = self.groups[grp][0]
        self.touched.add((base, window, d1 + 1))
        return pow(window_bases(b, p, self.w, self.windows)[window], d1 + 1, p)

    def verify(self, digest: bytes, sig: bytes, key: int = 0):
        key = min(key, len(self.keys) - 1)
        grp = self.keys[key][0]
        p, q, _ = self.groups[grp]
        status, decided, u1, u2, r = self.h.prep(sig, self.qbytes, q, digest)
        v, started = 0, False
        for base, e in ((grp, u1), (len(self.groups) + key, u2)):
            for i in range(self.windows):
                d = self.h.digit(e, i, self.w)
                if d:
                    t = self._entry(self.h.entry(base, i, d, self.windows, self.w))
                    v = v * t % p if started else t
                    started = True
        if not started:
            v = 1 % p
        rr = decode(r)
        return int(v % q == rr and not decided), status
