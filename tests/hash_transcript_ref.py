"""Test-side restatement of the reference's second transcript family: ShaRead / ShaWrite over a digest D
(halo2-snark-aggregator-api/src/transcript/sha.rs:23-232), with the method names of oracle/poseidon.py's transcript classes
so that oracle/verifier.py's build_params / verify_single_proof_no_eval take them as they are.

  read_point        64 bytes: x then y, 32-byte little-endian each; from_repr needs each < p, from_xy the curve; common_point
  read_scalar       32 bytes little-endian, < r; common_scalar
  common_point      update(31 zero bytes | 0x01 | x big-endian | y big-endian); the identity is an error
  common_scalar     update(31 zero bytes | 0x02 | scalar big-endian)
  squeeze           update(0x00); result = finalize(clone); state = D(result); challenge = LE(result | 32 zero bytes) mod r
                    (Challenge255::new -> from_bytes_wide: halo2_proofs, unvendored — recalled)

D = SHA-256 from hashlib, or Keccak-256 (the ORIGINAL padding 0x01 .. 0x80, rate 136 — not SHA3-256) from the pure-Python
Keccak-f[1600] below, which tests/test_hash_transcript_host.py pins against hashlib.sha3_256 (padding 0x06) and the published
Keccak-256 vectors."""
from __future__ import annotations

import hashlib

from oracle import bn254 as O
from oracle.poseidon import TranscriptError

R, P = O.R, O.P
_M64 = (1 << 64) - 1
_RHO = [0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14]   # index x + 5 y


def _rc():
    out, lfsr = [], 1
    for _ in range(24):
        rc = 0
        for j in range(7):
            if lfsr & 1:
                rc ^= 1 << ((1 << j) - 1)
            lfsr = ((lfsr << 1) ^ (0x71 if lfsr & 0x80 else 0)) & 0xFF
        out.append(rc)
    return out


_RC = _rc()


def _rotl(v, n):
    return ((v << n) | (v >> (64 - n))) & _M64 if n else v


def keccak_f1600(a):
    for rc in _RC:
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
        d = [c[(x + 4) % 5] ^ _rotl(c[(x + 1) % 5], 1) for x in range(5)]
        a = [a[i] ^ d[i % 5] for i in range(25)]
        b = [0] * 25
        for x in range(5):
            for y in range(5):
                b[y + 5 * ((2 * x + 3 * y) % 5)] = _rotl(a[x + 5 * y], _RHO[x + 5 * y])
        a = [b[i] ^ (~b[5 * (i // 5) + (i + 1) % 5] & _M64 & b[5 * (i // 5) + (i + 2) % 5]) for i in range(25)]
        a[0] ^= rc
    return a


def keccak_sponge256(msg: bytes, pad: int) -> bytes:
    """rate 136, capacity 512, 32 bytes out; pad = 0x01 (Keccak-256) or 0x06 (SHA3-256)"""
    rate = 136
    m = bytearray(msg)
    m.append(pad)
    m += bytes(-len(m) % rate)
    m[-1] |= 0x80
    a = [0] * 25
    for off in range(0, len(m), rate):
        for i in range(rate // 8):
            a[i] ^= int.from_bytes(m[off + 8 * i:off + 8 * i + 8], "little")
        a = keccak_f1600(a)
    return b"".join(v.to_bytes(8, "little") for v in a[:4])


def keccak256(msg: bytes) -> bytes:
    return keccak_sponge256(msg, 0x01)


class _Sha256:
    def __init__(self):
        self.h = hashlib.sha256()

    def update(self, b):
        self.h.update(b)

    def digest(self):
        return self.h.copy().digest()


class _Keccak256:
    def __init__(self):
        self.buf = bytearray()

    def update(self, b):
        self.buf += b

    def digest(self):
        return keccak256(bytes(self.buf))


DIGESTS = {"sha256": _Sha256, "keccak256": _Keccak256}


class _ShaTranscript:
    digest = "sha256"

    def _init_state(self):
        self.state = DIGESTS[self.digest]()
        self.absorbed = 0          # bytes in the current state (tests look at the padding boundaries they hit)
        self.squeezed_lengths = []

    def _update(self, b):
        self.state.update(b)
        self.absorbed += len(b)

    def common_point(self, pt):
        if pt is O.INF:
            raise TranscriptError("cannot write points at infinity to the transcript")
        self._update(bytes(31) + b"\x01" + pt[0].to_bytes(32, "big") + pt[1].to_bytes(32, "big"))

    def common_scalar(self, s: int):
        self._update(bytes(31) + b"\x02" + (s % R).to_bytes(32, "big"))

    def squeeze_challenge_scalar(self) -> int:
        self._update(b"\x00")
        result = self.state.digest()
        self.squeezed_lengths.append(self.absorbed)
        self.state = DIGESTS[self.digest]()
        self.absorbed = 0
        self._update(result)
        return int.from_bytes(result + bytes(32), "little") % R


class ShaTranscriptRead(_ShaTranscript):
    """ShaRead<_, _, Challenge255<_>, Sha256> over a byte string (sha.rs:23-127)"""

    def __init__(self, data: bytes):
        self._init_state()
        self.data, self.pos = data, 0

    def _take(self, n):
        if self.pos + n > len(self.data):
            raise TranscriptError("read_exact: unexpected end of proof")
        b = self.data[self.pos:self.pos + n]
        self.pos += n
        return b

    def read_point(self):
        x = int.from_bytes(self._take(32), "little")
        y = int.from_bytes(self._take(32), "little")
        if x >= P or y >= P:
            raise TranscriptError("invalid base encoding in proof")
        if (y * y - x * x * x - 3) % P != 0:
            raise TranscriptError("invalid point encoding in proof")
        self.common_point((x, y))
        return (x, y)

    def read_scalar(self) -> int:
        v = int.from_bytes(self._take(32), "little")
        if v >= R:
            raise TranscriptError("invalid field element encoding in proof")
        self.common_scalar(v)
        return v


class ShaTranscriptWrite(_ShaTranscript):
    """ShaWrite (sha.rs:129-232)"""

    def __init__(self):
        self._init_state()
        self.out = bytearray()

    def write_point(self, pt):
        self.common_point(pt)
        self.out += pt[0].to_bytes(32, "little") + pt[1].to_bytes(32, "little")

    def write_scalar(self, s: int):
        self.common_scalar(s)
        self.out += (s % R).to_bytes(32, "little")

    def finalize(self) -> bytes:
        return bytes(self.out)


class KeccakTranscriptRead(ShaTranscriptRead):
    digest = "keccak256"


class KeccakTranscriptWrite(ShaTranscriptWrite):
    digest = "keccak256"


READERS = {"sha256": ShaTranscriptRead, "keccak256": KeccakTranscriptRead}
WRITERS = {"sha256": ShaTranscriptWrite, "keccak256": KeccakTranscriptWrite}


def run_script(kind: str, proof: bytes, script: str, consts=(), ext_points=()):
    """the reference reader over one proof, driven by a P S Q C X script -> (points as 64-byte affine, challenges as 32 bytes)"""
    rd = READERS[kind](proof)
    pts, chal = [], []
    ci = xi = 0
    for ch in script:
        if ch == "P":
            pts.append(O.aff_to_bytes(rd.read_point()))
        elif ch == "S":
            rd.read_scalar()
        elif ch == "C":
            rd.common_scalar(consts[ci])
            ci += 1
        elif ch == "X":
            rd.common_point(ext_points[xi])
            xi += 1
        elif ch == "Q":
            chal.append(O.fe_to_bytes(rd.squeeze_challenge_scalar()))
    assert rd.pos == len(proof)
    return b"".join(pts), b"".join(chal), rd.squeezed_lengths
