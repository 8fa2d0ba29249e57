"""CPU: the epilogue of k_rsa_modexp<18,4,29> (csrc/kernels.hip) transcribed to Python -- the check of everything above bit
672 of the canonical 29-bit limbs against the 00 01 FF .. FF pattern (`em_head_limb<29>`, limb 23 from its bit 5 up) and the
re-cut of the low 672 bits into the 24 limbs of 28 bits k_rsa_compare reads -- held against real EMSA-PKCS1-v1_5 encodings
(oracle/openpgp.py's DigestInfo prefixes): every hash, moduli of 256 .. 2048 bits with k mod 4 = 0 .. 3, and each encoding
with one bit flipped on both sides of the split (671 | 672) and of limb 23 (666 | 667, 695).  A modulus of 256 .. 352 bits
holds no encoding of any hash (k < tLen + 11: k_parse_body refuses the signature before the kernel sees it); the shortest
that does is 45 bytes, under MD5."""
import hashlib

import pytest

from oracle import openpgp as O

W, NL = 29, 72
MASK29, MASK28 = (1 << 29) - 1, (1 << 28) - 1
EM_LOW_BYTES, EM_LOW_LIMBS = 84, 24
CUT = 8 * EM_LOW_BYTES
EM_HEAD_BAD = 0xFFFFFFFF
U32 = 0xFFFFFFFF

HASHES = ["md5", "sha1", "ripemd160", "sha224", "sha256", "sha384", "sha512"]
DLEN = {"md5": 16, "sha1": 20, "ripemd160": 20, "sha224": 28, "sha256": 32, "sha384": 48, "sha512": 64}
MOD_BITS = [256, 257, 264, 265, 273, 281, 360, 361, 369, 377, 385, 512, 672, 680, 696, 697, 1000, 1024, 1025, 1033, 1041, 1049, 1536, 2033, 2040, 2041, 2047, 2048]
FLIPS = [666, 667, 671, 672, 695]


def em_head_limb(gi, kbytes):
    top, lo = 8 * (kbytes - 2), gi * W
    if top < lo:
        return 0
    if top >= lo + W - 1:
        return MASK29
    return (1 << (top - lo + 1)) - 1


def epilogue(y, kbytes):
    """-> (head, out[24]): what the kernel's four writer lanes store for a canonical residue y < 2^2088."""
    limbs = [(y >> (W * i)) & MASK29 for i in range(NL)]
    head = 0
    for gi in range(NL):                                   # gi = qlane * 18 + k over the group's four lanes
        lo = gi * W
        if lo + W > CUT:
            d = limbs[gi] ^ em_head_limb(gi, kbytes)
            head |= (d >> (CUT - lo)) if lo < CUT else d
    out = []
    for j in range(EM_LOW_LIMBS):                          # j = qlane * 6 + k
        bit = 28 * j
        i, sh = bit // W, bit % W
        v = ((limbs[i] >> sh) | ((limbs[i + 1] << (W - sh)) & U32)) & MASK28
        out.append(EM_HEAD_BAD if (head != 0 and j == 0) else v)
    return head, out


def encodings():
    for h in HASHES:
        digest = hashlib.sha512(h.encode()).digest()[:DLEN[h]]
        t = O.HASH_PREFIXES[h] + digest
        for bits in MOD_BITS:
            k = (bits + 7) // 8
            if k < len(t) + 11:                            # rsa.VerifyPKCS1v15 refuses: k_parse_body never queues these
                continue
            em = b"\x00\x01" + b"\xff" * (k - len(t) - 3) + b"\x00" + t
            assert len(em) == k
            yield h, bits, k, int.from_bytes(em, "big")


def _low28(v):
    return [(v >> (28 * j)) & MASK28 for j in range(EM_LOW_LIMBS)]


def test_coverage():
    seen = {(h, k % 4) for h, _, k, _ in encodings()}
    assert seen == {(h, r) for h in HASHES for r in range(4)}
    ks = [k for _, _, k, _ in encodings()]
    assert min(ks) == 45 and max(ks) == 256 and any(k * 8 < CUT for k in ks) and any(CUT <= 8 * (k - 2) < CUT + 24 for k in ks)


def test_a_true_encoding_passes_the_head_and_leaves_its_low_limbs():
    for h, bits, k, em in encodings():
        head, out = epilogue(em, k)
        assert head == 0, (h, bits)
        assert out == _low28(em), (h, bits)


@pytest.mark.parametrize("bit", FLIPS)
def test_one_flipped_bit(bit):
    for h, bits, k, em in encodings():
        y = em ^ (1 << bit)
        head, out = epilogue(y, k)
        if bit < CUT:                                      # k_rsa_compare's side: the head holds, exactly that bit differs below
            assert head == 0, (h, bits)
            assert out == _low28(y) and out != _low28(em), (h, bits)
        else:                                              # the kernel's side: marked, whatever the low limbs are
            assert head != 0 and out[0] == EM_HEAD_BAD, (h, bits)
            assert out[1:] == _low28(em)[1:], (h, bits)


def test_verdict_is_equality_with_the_encoding():
    """head == 0 and the 24 limbs equal the encoding's <=> y is the encoding: over values that differ from it in one bit at
    every position of limbs 22 .. 24 and at the top, and by +-n-like offsets high and low."""
    for h, bits, k, em in encodings():
        ys = [em ^ (1 << b) for b in list(range(22 * W, 25 * W)) + [0, 27, 28, 29, 8 * k - 16, 8 * k - 9, 8 * k - 8, 8 * k - 1, 8 * k, 2087]]
        ys += [em + (1 << CUT), em - 1, em + 1]
        if em >= 1 << CUT:
            ys.append(em - (1 << CUT))
        for y in ys:
            head, out = epilogue(y, k)
            assert (head == 0 and out == _low28(em)) == (y == em), (h, bits, hex(y ^ em))
