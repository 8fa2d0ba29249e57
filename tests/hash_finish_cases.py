"""The hash finish at every padding boundary: the case set shared by tests/test_hash_finish_reference.py (the two oracles agree on
it; it covers what it claims to cover) and tests/test_gpu_hash_finish.py (the device agrees with the oracle on it).

The device builds a digest in two steps (bftkv_amd/csrc/kernels.hip): a per-item midstate over the whole blocks of the hashed
stream (k_sha256_mid, k_hash_mid_other, k_hash_mid_text; host_sha256.h for the staged calls), and a per-signature finish
(digest_body) that rebuilds the last blocks byte by byte (tail_byte) from the stream's last n mod B bytes, the signature's own
suffix and the padding.  With B the block size (64; 128 for SHA-384 / SHA-512), L the size of the length field (8; 16), n the
length of the stream hashed before the suffix (the payload, or its canonical-text form) and unit the suffix length (12 + hl for a
v4 signature, 5 for v3), everything the finish decides depends on rem = (n mod B) + unit: the number of finish blocks
ceil((rem + 1 + L) / B), the word that takes the 0x80 marker, the words the trailer 04 FF len32 straddles, and the overwrite of
the last block's length words (big-endian, or little-endian for MD5 / RIPEMD-160).  The BOUNDARY RESIDUES of rem mod B are
B-L-2, B-L-1, B-L, B-L+1 (the length field just fits / just does not), B-1, 0 and 1 (the marker at the end of a block, at the
start of the next).

Every signature is made with the corpus's 1024-bit RSA key: with k = 128 the digest of every hash, SHA-512 included, lies inside
the 84 low bytes of the encoded message that k_rsa_compare rebuilds from the device's digest, so a valid signature verifies only
if that digest is exact in every byte.  Reference digests come from hashlib, from the oracle's RIPEMD-160 (hashlib here has none;
tests/golden/gpg_weak_hash_vectors.json pins it) and from the oracle's CanonicalTextHash.

Groups (each case records hash, kind, n, unit, rem):
  A  every residue: all seven hashes, v4 binary, the plain hashed area (hl = 16, unit = 28), payload lengths B .. 2B-1 -- one whole
     block, so the midstate is never the initial value;
  B  whole-block counts and load alignment: lengths k B + {0, 1, B-1} for k = 0 .. 5; for the four block loaders (SHA-256's
     two-blocks-per-trip loop, SHA-1, MD5, SHA-512) every k = 1 .. 5 at every payload start offset mod 4 -- layout() puts 1-3-byte
     filler items with an empty signature stream in front of such a case -- and the LAST item of the blob is a misaligned payload of
     whole blocks only (the 17th dword of its last block lies in the 64 bytes by which the host entry points pad their staging);
  C  suffix length: unit in {28, 30, 31, 33}, {60 .. 63}, {124 .. 127} (each set covers the four word alignments of the marker and
     the trailer), 312 (a two-octet subpacket length) and 65,547 (hl = 65,535, the largest there is: docs/parity.md names no size
     above which a definite-length signature whose fetches end at its packet's end is fenced), the hashed area stretched by
     non-critical notation subpackets; under each unit every tail < B that puts rem mod B on a boundary residue, alternately over no
     whole block and one;
  D  v3 signatures (unit = 5, no trailer): every residue for SHA-256 and SHA-512, the boundary residues for the other five;
  E  text mode (type 0x01), n = the canonical length: every residue for SHA-256 and SHA-512 over payloads that mix bare LFs, CRLFs
     and lone CRs; for all seven hashes the boundary residues under bare LFs only (every one expands), CRLFs already present and a
     trailing lone CR (nothing expands), and a bare LF placed so that the inserted CR is the last byte of a block and the LF the
     first of the next ("edge"), and the same one byte later ("edge+1");
  F  negative twins: every eighth case once more over its payload with one bit flipped -- in turn the first byte, the last byte of
     the last whole block, the first byte of the tail, the last byte (the next of these that exists).  Expected: what the oracle says.
2,027 signatures and 254 twins; cases() is deterministic, cached, and takes about 7 s of one CPU core (2 ms per CRT signature and
the oracle's Python RIPEMD-160 over the seven 65 KB suffixes) -- nothing had to be thinned.
"""
from __future__ import annotations

import functools
import hashlib
import struct
from contextlib import contextmanager
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from corpus import build as cb
from corpus.keys import load_keys
from oracle import collective as col
from oracle import openpgp as pgp
from oracle.packet import SignaturePacket
from tests import rsa_sizes as RS

HASHES: List[Tuple[int, str]] = [(1, "md5"), (2, "sha1"), (3, "ripemd160"), (11, "sha224"), (8, "sha256"), (9, "sha384"), (10, "sha512")]
NAMES: Dict[int, str] = dict(HASHES)
LOADERS = (8, 2, 1, 10)             # k_sha256_mid; load_block_be (SHA-1); load_block_le (MD5); two load_block_be per block (SHA-512)
K = 128                             # byte length of the signing key's modulus
PLAIN_UNIT = 28                     # 6 + 16 hashed bytes (creation time, issuer) + the 6-byte trailer
UNIT_SETS: List[Tuple[int, ...]] = [(28, 30, 31, 33), (60, 61, 62, 63), (124, 125, 126, 127), (312,), (12 + 65535,)]
UNITS = [u for s in UNIT_SETS for u in s]
TEXT_SHAPES = ("lf", "crlf", "edge", "edge+1")
TWIN_EVERY = 8


def b_tails(B: int) -> Tuple[int, int, int]:
    return (0, 1, B - 1)


def block(hash_id: int) -> int:
    return 128 if hash_id in (9, 10) else 64


def len_field(hash_id: int) -> int:
    return 16 if hash_id in (9, 10) else 8


def boundary_residues(hash_id: int) -> List[int]:
    B, L = block(hash_id), len_field(hash_id)
    return [B - L - 2, B - L - 1, B - L, B - L + 1, B - 1, 0, 1]


def finish_blocks(hash_id: int, rem: int) -> int:
    """Blocks behind the midstate: rem bytes, the marker and the length field."""
    B = block(hash_id)
    return (rem + 1 + len_field(hash_id) + B - 1) // B


@dataclass(frozen=True)
class Case:
    group: str                       # "A" .. "E"; a twin keeps the group of its positive
    hash_id: int
    kind: str                        # "v4" | "v3" | "text"
    n: int                           # length of the stream hashed before the suffix
    unit: int
    rem: int
    tbs: bytes
    sig: bytes                       # one signature packet
    detail: str = ""                 # E: the payload shape
    k: Optional[int] = None          # B: whole blocks
    want_off: Optional[int] = None   # B: payload start offset mod 4 that layout() gives it
    last: bool = False               # B: goes to the end of the payload blob
    twin_of: Optional[int] = None    # F: index of the positive
    flipped: Optional[str] = None    # F: which byte

    @property
    def label(self):
        return (NAMES[self.hash_id], self.kind, self.n, self.unit, self.rem) + ((self.flipped,) if self.flipped else ())


@functools.lru_cache(maxsize=None)
def keypair() -> cb.KeyPair:
    kp = cb.make_keypair(cb.PK_RSA, load_keys("rsa1024", 1)[0], "hash finish <k@bftkv.example>")
    assert kp.n.bit_length() == 8 * K
    return kp


def keyring() -> col.Keyring:
    return col.Keyring(keyring=[RS.entity(keypair())])


@contextmanager
def weak_hashes_available():
    """The oracle's policy for MD5 / RIPEMD-160 set to "linked" for the duration."""
    saved = dict(pgp.HASH_POLICY)
    pgp.HASH_POLICY.update(md5=True, ripemd160=True)
    try:
        yield
    finally:
        pgp.HASH_POLICY.update(saved)


def fill(tag: str, n: int) -> bytes:
    return hashlib.shake_128(tag.encode()).digest(n) if n else b""


_LETTERS = b"abcdefghijklmnopqrstuvwxyz ,.;"


def letters(tag: str, n: int) -> bytes:
    return bytes(_LETTERS[b % len(_LETTERS)] for b in fill(tag, n))


class _Collect:
    def __init__(self):
        self.b = bytearray()

    def update(self, data: bytes):
        self.b += data


def canonical(payload: bytes) -> bytes:
    """The bytes the oracle's CanonicalTextHash hands to the hash."""
    c = _Collect()
    pgp.CanonicalTextHash(c).update(payload)
    return bytes(c.b)


def stretch(m: int, tag: str) -> bytes:
    """Non-critical notation subpackets (type 20) of m bytes in all, length octets included."""
    if m == 0:
        return b""
    if 2 <= m <= 192:
        return bytes([m - 1, 20]) + fill(tag, m - 2)
    if 192 <= m - 2 < 8384:
        return bytes([((m - 2 - 192) >> 8) + 192, (m - 2 - 192) & 0xFF, 20]) + fill(tag, m - 3)
    assert m >= 6
    return b"\xff" + struct.pack(">I", m - 5) + bytes([20]) + fill(tag, m - 6)


def text_payload(shape: str, hash_id: int, target: int) -> bytes:
    """A payload of the shape whose canonical form has ``target`` bytes."""
    B = block(hash_id)
    tag = "text %s %d %d" % (shape, hash_id, target)
    fillers = letters(tag, target + 2)
    out = bytearray()
    if shape in ("lf", "crlf"):
        end = target - (shape == "crlf")                # crlf: room for the trailing lone CR
        clen = i = 0
        while clen < end:
            if i % 5 == 4 and clen + 2 < end:           # (never the last thing: a crlf payload ends letter, CR)
                out += b"\n" if shape == "lf" else b"\r\n"
                clen += 2
            else:
                out.append(fillers[i])
                clen += 1
            i += 1
        if shape == "crlf":
            out += b"\r"
    elif shape in ("edge", "edge+1"):
        at = B - 1 + (shape == "edge+1")
        assert target >= at + 2
        out += fillers[:at] + b"\n" + letters(tag + " behind", target - at - 2)
    else:                                               # "mixed"
        tokens = [b"ab", b"\n", b"cd\r\n", b"e\rf", b"\r\r\n", b"\n\n", b"g\r"]
        i = 0
        while len(canonical(bytes(out))) < target:
            t = tokens[(i + target) % len(tokens)]
            if len(canonical(bytes(out) + t)) > target:
                t = fillers[i % len(fillers):][:1]
            out += t
            i += 1
    assert len(canonical(bytes(out))) == target, (shape, hash_id, target)
    return bytes(out)


def stream_len(kind: str, tbs: bytes) -> int:
    return len(canonical(tbs)) if kind == "text" else len(tbs)


def _sign(group: str, hash_id: int, kind: str, tbs: bytes, extra: bytes = b"", **kw) -> Case:
    kp, name = keypair(), NAMES[hash_id]
    if kind == "v3":
        prefix = None
        suffix = bytes([0]) + struct.pack(">I", cb.CREATION_TIME)                   # type || creation time, no trailer
    else:
        prefix = cb.sig_prefix(0x01 if kind == "text" else 0x00, cb.PK_RSA, cb._hashed_area(kp.key_id, extra), hash_id)
        suffix = cb.hash_suffix(prefix)
    h = pgp.CanonicalTextHash(pgp.new_hash(name)) if kind == "text" else pgp._BinaryHash(pgp.new_hash(name))
    h.update(tbs)
    h.raw_update(suffix)
    digest = h.digest()
    mpi = RS.go_mpi(kp.rsa_private(int.from_bytes(RS.encode(K, name, digest), "big")), K)
    if kind == "v3":
        body = bytes([3, 5]) + suffix + struct.pack(">Q", kp.key_id) + bytes([cb.PK_RSA, hash_id]) + digest[:2] + mpi
        sig = cb._hdr(2, len(body)) + body
    else:
        sig = RS.packet(prefix, digest, mpi)
    n = stream_len(kind, tbs)
    return Case(group, hash_id, kind, n, len(suffix), n % block(hash_id) + len(suffix), tbs, sig, **kw)


def _twin(i: int, c: Case, turn: int) -> Case:
    B, ln = block(c.hash_id), len(c.tbs)
    whole = ln // B * B
    places = [("first byte", 0), ("last byte of the last whole block", whole - 1 if whole else None),
              ("first byte of the tail", whole if whole < ln else None), ("last byte", ln - 1)]
    name, at = next(p for p in (places[(turn + j) % 4] for j in range(4)) if p[1] is not None)
    tbs = bytearray(c.tbs)
    tbs[at] ^= 0x01
    n = stream_len(c.kind, bytes(tbs))
    return Case(c.group, c.hash_id, c.kind, n, c.unit, n % B + c.unit, bytes(tbs), c.sig, c.detail, c.k, None, False, i, name)


@functools.lru_cache(maxsize=None)
def cases() -> List[Case]:
    out: List[Case] = []
    for hash_id, _ in HASHES:                                   # ---- A
        B = block(hash_id)
        for n in range(B, 2 * B):
            out.append(_sign("A", hash_id, "v4", fill("A %d %d" % (hash_id, n), n)))
    for hash_id, _ in HASHES:                                   # ---- B
        B = block(hash_id)
        for k in range(6):
            for j, d in enumerate(b_tails(B)):
                want = (k + j) % 4 if hash_id in LOADERS and k else None
                out.append(_sign("B", hash_id, "v4", fill("B %d %d %d" % (hash_id, k, d), k * B + d), k=k, want_off=want))
            if hash_id in LOADERS and k:                        # the fourth offset: whole blocks only, another payload
                out.append(_sign("B", hash_id, "v4", fill("B4 %d %d" % (hash_id, k), k * B), k=k, want_off=(k + 3) % 4))
        if hash_id in LOADERS:
            out.append(_sign("B", hash_id, "v4", fill("B last %d" % hash_id, 3 * B), k=3, want_off=1 + hash_id % 3, last=True))
    for hash_id, _ in HASHES:                                   # ---- C
        B = block(hash_id)
        for ui, unit in enumerate(UNITS):
            extra = stretch(unit - PLAIN_UNIT, "C %d %d" % (hash_id, unit))
            for ri, r in enumerate(boundary_residues(hash_id)):
                n = (r - unit) % B + B * ((ui + ri) % 2)
                c = _sign("C", hash_id, "v4", fill("C %d %d %d" % (hash_id, unit, r), n), extra)
                assert c.unit == unit and c.rem % B == r
                out.append(c)
    for hash_id, _ in HASHES:                                   # ---- D
        B = block(hash_id)
        for r in (range(B) if hash_id in (8, 10) else boundary_residues(hash_id)):
            n = B + (r - 5) % B
            out.append(_sign("D", hash_id, "v3", fill("D %d %d" % (hash_id, n), n)))
    for hash_id, _ in HASHES:                                   # ---- E
        B = block(hash_id)
        if hash_id in (8, 10):
            for n in range(B, 2 * B):
                out.append(_sign("E", hash_id, "text", text_payload("mixed", hash_id, n), detail="mixed"))
        for shape in TEXT_SHAPES:
            for r in boundary_residues(hash_id):
                n = (r - PLAIN_UNIT) % B + B                     # the canonical length; the edge shapes need B + 2 at the least
                if shape.startswith("edge") and n < B + 3:
                    n += B
                out.append(_sign("E", hash_id, "text", text_payload(shape, hash_id, n), detail=shape))
    twins: List[Case] = []                                      # ---- F
    due = False
    for i, c in enumerate(out):
        due = due or i % TWIN_EVERY == 0
        if due and c.tbs:
            twins.append(_twin(i, c, len(twins)))
            due = False
    return out + twins


def oracle_verdict(kr: col.Keyring, c: Case) -> Tuple[bool, List[int]]:
    """(accepted, per-packet statuses) of PGPSignature.Verify; call under weak_hashes_available()."""
    tr: List[int] = []
    err = col.signature_verify(kr, c.tbs, SignaturePacket(1, 0, False, c.sig, None), trace=tr)
    return err is None, tr


# ---- the orders in which the GPU test submits the set, and the item lists they become
def shuffled_order() -> List[int]:
    return [int(i) for i in np.random.default_rng(20260).permutation(len(cases()))]


def by_hash_order() -> List[int]:
    cs = cases()
    rank = {h: j for j, (h, _) in enumerate(HASHES)}
    return sorted(range(len(cs)), key=lambda i: (rank[cs[i].hash_id], cs[i].kind, i))


def sha256_binary_order() -> List[int]:
    return [i for i, c in enumerate(cases()) if c.hash_id == 8 and c.kind == "v4"]


@dataclass
class Layout:
    tbs: List[bytes]                 # one payload per item, fillers included
    sig: List[bytes]                 # b"" for a filler
    case: List[Optional[int]]        # the case of each item; None: a filler
    start: List[int]                 # offset of each item's payload in the blob


def layout(order: Sequence[int]) -> Layout:
    """The items of one call: the cases in ``order``, the ``last`` ones moved to the end, and a filler item of 1-3 bytes with an
    empty signature stream in front of every case that asks for a payload start offset mod 4 it would not get otherwise."""
    cs = cases()
    order = [i for i in order if not cs[i].last] + [i for i in order if cs[i].last]
    lay = Layout([], [], [], [])
    cur = 0

    def put(tbs, sig, ci):
        nonlocal cur
        lay.tbs.append(tbs); lay.sig.append(sig); lay.case.append(ci); lay.start.append(cur)
        cur += len(tbs)
    for i in order:
        want = cs[i].want_off
        if want is not None and cur % 4 != want:
            put(b"\xa5" * ((want - cur) % 4), b"", None)
        put(cs[i].tbs, cs[i].sig, i)
    return lay
