"""The message set of the multi-message tests, picked once on the CPU with
hashlib: for each length around SHA-256's one- and two-block padding
boundaries at least one message whose digest is a valid hashedMessage scalar
(0 < digest < Order) and one that is "EOF" (digest 0 or >= Order, about 44 %
of messages), plus the empty message, which is EOF."""

import hashlib

ORDER = 65000549695646603732796438742359905742570406053903786389881062969044166799969
LENGTHS = (1, 55, 56, 63, 64, 65, 119, 120, 200)


def digest_int(msg: bytes) -> int:
    return int.from_bytes(hashlib.sha256(msg).digest(), "big")


def hashable(msg: bytes) -> bool:
    return 0 < digest_int(msg) < ORDER


def message(length: int, seed: int) -> bytes:
    out, ctr = b"", 0
    while len(out) < length:
        out += hashlib.sha256(b"msgs-fixture:%d:%d:%d" % (length, seed, ctr)).digest()
        ctr += 1
    return out[:length]


def boundary_set():
    """[(msg, hashable)]: per length the first hashable and the first EOF
    message over the seeds 0.., then the empty message."""
    out = []
    for length in LENGTHS:
        found = {}
        for seed in range(64):
            m = message(length, seed)
            found.setdefault(hashable(m), m)
            if len(found) == 2:
                break
        out += [(found[h], h) for h in (True, False) if h in found]
    out.append((b"", hashable(b"")))
    return out


def check_boundary_set(msgs):
    """A bad set fails loudly instead of testing nothing."""
    for length in LENGTHS:
        kinds = {h for m, h in msgs if len(m) == length}
        assert kinds == {True, False}, (length, kinds)
    assert (b"", False) in msgs
    for m, h in msgs:
        assert h == hashable(m)
