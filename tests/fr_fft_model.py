"""Integer model of the transform over Fr that Engine.fr_fft computes,

    out[j] = post^j * scale * sum_i pre^i * a_i * w^(i j)   (mod r),

for the tests of the scalar FFT: the definition as a double loop for n <= 64, a recursive radix-2 evaluation for larger
n (checked against the double loop in the CPU suite), and the two record forms -- plain integers and libff's Montgomery
residues with R = 2^(32 words).  Python integers only; the moduli come from amdmsm_fr_modulus.  Nothing here knows of
tiles, passes or the order of the butterflies."""
import random

import numpy as np

CURVES = {0: "alt_bn128", 1: "bls12_377", 2: "bw6_761", 3: "bls12_381", 4: "mnt4", 5: "mnt6"}
TWO_ADICITY = {0: 28, 1: 47, 2: 46, 3: 32, 4: 34, 5: 17}
# Fr::multiplicative_generator of the reference's <curve>_init.cpp (tests/golden/fr_domain.npz holds them too)
GENERATOR = {0: 5, 1: 22, 2: 15, 3: 7, 4: 10, 5: 17}

_fields = {}


class Field:
    def __init__(self, curve):
        import libff_amd

        self.curve = curve
        self.r = libff_amd.fr_modulus(curve, libff_amd.G1)
        self.words = libff_amd.sizes(curve, libff_amd.G1)["fr_bytes"] // 4
        self.limbs = self.words // 2
        self.R = 1 << (32 * self.words)
        self.s = TWO_ADICITY[curve]

    def records(self, values, plain):
        """(n, limbs) uint64 records of the integers `values`"""
        buf = bytearray()
        for v in values:
            v %= self.r
            buf += (v if plain else v * self.R % self.r).to_bytes(8 * self.limbs, "little")
        return np.frombuffer(bytes(buf), dtype="<u8").astype(np.uint64).reshape(len(values), self.limbs)

    def ints(self, records, plain):
        rinv = pow(self.R, -1, self.r)
        out = []
        for row in np.ascontiguousarray(records, dtype="<u8"):
            v = int.from_bytes(row.tobytes(), "little")
            out.append(v if plain else v * rinv % self.r)
        return out

    def root(self, n):
        """a primitive n-th root of unity from the field's generator (the one get_root_of_unity gives)"""
        assert n & (n - 1) == 0 and n <= 1 << self.s
        return pow(GENERATOR[self.curve], (self.r - 1) // n, self.r)


def field(curve):
    if curve not in _fields:
        _fields[curve] = Field(curve)
    return _fields[curve]


def naive(a, w, r, pre=1, post=1, scale=1):
    """the definition, n^2 products: n <= 64"""
    n = len(a)
    assert n <= 64
    out = []
    for j in range(n):
        acc = 0
        for i in range(n):
            acc += pow(pre, i, r) * a[i] * pow(w, i * j, r)
        out.append(pow(post, j, r) * scale * acc % r)
    return out


def _rec(a, w, r):
    n = len(a)
    if n == 1:
        return list(a)
    even, odd = _rec(a[0::2], w * w % r, r), _rec(a[1::2], w * w % r, r)
    out, t = [0] * n, 1
    for j in range(n // 2):
        x = t * odd[j] % r
        out[j], out[j + n // 2] = (even[j] + x) % r, (even[j] - x) % r
        t = t * w % r
    return out


def fft(a, w, r, pre=1, post=1, scale=1):
    """the same values by recursive halving (w a primitive len(a)-th root of unity)"""
    n = len(a)
    if n == 0:
        return []
    x, f = [], 1
    for v in a:
        x.append(v * f % r)
        f = f * pre % r
    y, out, f = _rec(x, w % r, r), [], scale % r
    for v in y:
        out.append(v * f % r)
        f = f * post % r
    return out


_vectors = {}


def random_vector(curve, n, seed=0):
    """n canonical values, computed once per (curve, n, seed) and never changed"""
    key = (curve, n, seed)
    if key not in _vectors:
        rng = random.Random(1000003 * curve + 31 * n + seed)
        r = field(curve).r
        _vectors[key] = tuple(rng.randrange(r) for _ in range(n))
    return list(_vectors[key])
