"""The reference of the lossy UTF-8 tests (test code only): bytes.decode("utf-8", "replace") rebuilt from CPython's STRICT decoder,
so that it also says which bytes every unit of the result stands for.  The loop: decode strictly; on UnicodeDecodeError take what
decoded before .start, put one U+FFFD for the bytes [.start, .end) -- the maximal ill-formed subpart -- and go on at .end.  Nothing
here calls the product."""
import numpy as np

# the rows of the table in include/acgpu.h's lossy section: bytes -> the spans that become one U+FFFD each
TABLE = [(b"\xe0\x80\x80", [(0, 1), (1, 2), (2, 3)]),
         (b"\xed\xa0\x80", [(0, 1), (1, 2), (2, 3)]),
         (b"\xf4\x90\x80\x80", [(0, 1), (1, 2), (2, 3), (3, 4)]),
         (b"\xc0\xaf", [(0, 1), (1, 2)]),
         (b"\xf5", [(0, 1)]),
         (b"\xf0\x9f\x98", [(0, 3)]),                 # at the end of the text
         (b"\xf0\x9f\x28", [(0, 2)]),                 # then "("
         (b"\x61\xe2\x82", [(1, 3)]),                 # at the end
         (b"\xe2\x82\xe2\x82\xac", [(0, 2)]),         # then the euro sign
         (b"\xf0\x9f\x98\xf0\x9f\x98\x80", [(0, 3)])]  # then U+1F600
ALPHABET = bytes.fromhex("41 28 80 BF 9F 8F 90 A0 C0 C2 C3 E0 E2 82 ED F0 F4 F5")


def decode_replace(data):
    """-> (text, off, length, replaced): the decoded text, and per UTF-16 UNIT of it the byte offset and the byte length of what it
    stands for (both units of a surrogate pair: the four bytes of their code point; a U+FFFD that replaces a subpart: the
    subpart) and whether it is such a replacement"""
    data = bytes(data)
    parts, off, length, replaced = [], [], [], []

    def good(lo, text):
        cps = np.frombuffer(text.encode("utf-32-le"), dtype=np.uint32).astype(np.int64)
        nbytes = 1 + (cps >= 0x80) + (cps >= 0x800) + (cps >= 0x10000)
        units = 1 + (cps >= 0x10000)
        off.append(np.repeat(lo + np.cumsum(nbytes) - nbytes, units))
        length.append(np.repeat(nbytes, units))
        replaced.append(np.zeros(int(units.sum()), bool))
        parts.append(text)

    pos = 0
    while pos < len(data):
        try:
            good(pos, data[pos:].decode("utf-8"))
            break
        except UnicodeDecodeError as e:
            good(pos, data[pos:pos + e.start].decode("utf-8"))
            off.append(np.array([pos + e.start]))
            length.append(np.array([e.end - e.start]))
            replaced.append(np.ones(1, bool))
            parts.append("\ufffd")
            pos += e.end
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    return "".join(parts), cat(off, np.int64), cat(length, np.int64), cat(replaced, bool)


def spans(data):
    """the replaced subparts of `data` as (start, end) byte spans"""
    _, off, length, replaced = decode_replace(data)
    return [(int(o), int(o + n)) for o, n in zip(off[replaced], length[replaced])]


def damaged(rng, valid, n_buffers=200, max_len=300):
    """n_buffers buffers of 0 .. max_len bytes: runs over ALPHABET mixed with slices of the well-formed bytes `valid` (cut
    anywhere, inside sequences too)"""
    out = []
    for _ in range(n_buffers):
        want, buf = int(rng.integers(0, max_len + 1)), bytearray()
        while len(buf) < want:
            if rng.integers(3) == 0:
                i = int(rng.integers(len(valid) - 40))
                buf += valid[i:i + int(rng.integers(1, 40))]
            else:
                buf += bytes(ALPHABET[int(i)] for i in rng.integers(0, len(ALPHABET), int(rng.integers(1, 12))))
        out.append(bytes(buf[:want]))
    return out
