"""A plain-Python restatement of Go 1.13's rsa.VerifyPKCS1v15 on raw inputs with the rules of docs/parity.md ("RSA verification"),
for the RSA-verification tests.  Not collected.

    verify(n, e, hash_id, digest, s) -> (valid, status)

hash_id is an OpenPGP hash id, or 0 for no prefix; the caller checks len(digest) == DLEN[hash_id] (the device refuses the call).  The
rows, in this order, with k = ceil(bits(n) / 8) and tLen = len(prefix) + len(digest):
  1. k < tLen + 11 (n = 0 and n = 1 included): (0, OK) -- Go refuses before any arithmetic, whatever n's parity;
  2. n even: (0, FENCED) -- big.Int.Exp answers, the Montgomery rows cannot; no answer is claimed;
  3. m = s^e mod n for ANY s (Go <= 1.13 checks neither s < n nor the signature's length) and any e (e = 0 gives 1), em = m
     left-padded to k bytes: (em == 00 01 FF .. FF 00 || prefix || digest, OK)."""
OK, FENCED = 0, 2
PREFIX = {0: b"", 1: bytes.fromhex("3020300c06082a864886f70d020505000410"), 2: bytes.fromhex("3021300906052b0e03021a05000414"),
          3: bytes.fromhex("30203008060628cf060300310414"),          # Go's identifier for RIPEMD-160, not the one gpg writes
          8: bytes.fromhex("3031300d060960864801650304020105000420"), 9: bytes.fromhex("3041300d060960864801650304020205000430"),
          10: bytes.fromhex("3051300d060960864801650304020305000440"), 11: bytes.fromhex("302d300d06096086480165030402040500041c")}
DLEN = {1: 16, 2: 20, 3: 20, 8: 32, 9: 48, 10: 64, 11: 28}


def em(k: int, hash_id: int, digest: bytes) -> bytes:
    t = PREFIX[hash_id] + digest
    return b"\x00\x01" + b"\xff" * (k - len(t) - 3) + b"\x00" + t


def rule(n: int, hash_id: int, dlen: int) -> int:
    """0: the arithmetic row, 1: row 1, 2: row 2."""
    if (n.bit_length() + 7) // 8 < len(PREFIX[hash_id]) + dlen + 11:
        return 1
    return 2 if n % 2 == 0 else 0


def verify(n: int, e: int, hash_id: int, digest: bytes, s: int):
    r = rule(n, hash_id, len(digest))
    if r:
        return 0, (FENCED if r == 2 else OK)
    k = (n.bit_length() + 7) // 8
    return int(pow(s, e, n).to_bytes(k, "big") == em(k, hash_id, digest)), OK
