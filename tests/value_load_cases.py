"""What the value-loader tests share (csrc/value_load.h): the five lane forms of k_rsa_modexp and the limbs of a big-endian
byte string by plain integer slicing."""

FORMS = [(18, 4, 29), (19, 4, 28), (10, 8, 28), (14, 8, 28), (19, 8, 28)]      # (L, TPI, W), the order of the drivers under tests/c


def limbs(value_be, L, TPI, W):
    """The TPI * L radix-2^W limbs of the value, least significant first; what lies above them is dropped."""
    x = int.from_bytes(value_be, "big")
    mask = (1 << W) - 1
    return [(x >> (j * W)) & mask for j in range(L * TPI)]


def contents(nb, rng):
    """Random, all FF, all 00, and one set bit at either end."""
    out = [rng.bytes(nb), b"\xff" * nb, b"\x00" * nb]
    if nb:
        out.append(b"\x80" + b"\x00" * (nb - 1))
        out.append(b"\x00" * (nb - 1) + b"\x01")
    return out
