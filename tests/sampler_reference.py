"""A third statement of the HaltonSampler's arithmetic, in plain Python. Test infrastructure only.

The device's sampler (device/dmath.hpp, host/sampler_tables.cpp) and the oracle's (oracle/rrt_oracle.cpp) were written by the same hand. This one is
written from samplers/halton.rs and lowdiscrepancy.rs on its own: digits, indices, pixel offsets and the modular inverse are Python integers, which do
not overflow, and the power of the inverse base is a Python float multiplied once per digit, in the reference's order.

From a scene description it takes the film's size, `sample_at_center` and the digit permutation table (seeded, so not reproducible otherwise).
Everything else it derives - base scales and exponents, the stride, the two modular inverses, the prime table and its prefix sums - and check_desc()
holds what it derived against the description's own fields (host/halton_host.cpp, host/scene_loader.cpp).

What the reference does that a textbook would not, kept on purpose:
  * get_index_for_sample reverses base_exponents[1] digits of the x pixel too (halton.rs:91), so the first dimension names the
    pixel only where base_exponents[0] <= base_exponents[1];
  * extended_gcd's base case sets y = 1, not 0 (halton.rs:131-143): x is what the inverse uses, and x does not depend on it;
  * multiplicative_inverse casts the signed x to u64 before the modulo (halton.rs:149): a negative x becomes 2^64 + x first, and 2^64 is not a
    multiple of a power of 3;
  * dimensions 0 and 1 are not scrambled, and `index / base_scale` rather than `index` goes into them (halton.rs:117-120).
"""
import numpy as np

K_MAX_RESOLUTION = 128
PRIME_TABLE_SIZE = 1000
ONE_MINUS_EPSILON = 1.0 - 2.0 ** -53
POW_2_M64 = 2.0 ** -64
assert POW_2_M64 == float("0.00000000000000000005421010862427522") and ONE_MINUS_EPSILON == 0.99999999999999989


def first_primes(n):
    out, c = [], 2
    while len(out) < n:
        if all(c % p for p in out if p * p <= c): out.append(c)
        c += 1
    return out


PRIMES = first_primes(PRIME_TABLE_SIZE)
PRIME_SUMS = [sum(PRIMES[:i]) for i in range(PRIME_TABLE_SIZE)]      # where a dimension's permutation starts in the table


def extended_gcd(a, b):
    if b == 0: return 1, 1
    xp, yp = extended_gcd(b, a % b)
    return yp, xp - (a // b) * yp


def multiplicative_inverse(a, n):
    x, _ = extended_gcd(a, n)
    return (x % 2 ** 64) % n      # `x as u64`, then mod_t on u64


def inverse_radical_inverse(base, inverse, n_digits):
    index = 0
    for _ in range(n_digits):
        inverse, digit = divmod(inverse, base)
        index = index * base + digit
    return index


def reverse_bits_64(a):
    return int(format(a, "064b")[::-1], 2)


def radical_inverse(base_index, a):
    if base_index == 0: return float(reverse_bits_64(a)) * POW_2_M64
    base = PRIMES[base_index]
    inv_base, inv_base_n, reversed_digits = 1.0 / base, 1.0, 0
    while a != 0:
        a, digit = divmod(a, base)
        reversed_digits = reversed_digits * base + digit
        inv_base_n *= inv_base
    return min(float(reversed_digits) * inv_base_n, ONE_MINUS_EPSILON)


def scrambled_radical_inverse(base_index, a, perm):
    """perm: the permutation of this base's digits (the table from PRIME_SUMS[base_index] on)"""
    base = PRIMES[base_index]
    inv_base, inv_base_n, reversed_digits = 1.0 / base, 1.0, 0
    while a > 0:
        a, digit = divmod(a, base)
        reversed_digits = reversed_digits * base + perm[digit]
        inv_base_n *= inv_base
    return min(inv_base_n * (float(reversed_digits) + inv_base * float(perm[0]) / (1.0 - inv_base)), ONE_MINUS_EPSILON)


class Halton:
    def __init__(self, xres, yres, sample_at_center, perms):
        self.res = (int(xres), int(yres))
        self.sample_at_center = bool(sample_at_center)
        self.perms = [int(v) for v in perms]
        assert len(self.perms) == sum(PRIMES)
        self.base_scales, self.base_exponents = [], []
        for i, base in enumerate((2, 3)):
            scale, exp = 1, 0
            while scale < min(self.res[i], K_MAX_RESOLUTION):
                scale *= base; exp += 1
            self.base_scales.append(scale); self.base_exponents.append(exp)
        self.sample_stride = self.base_scales[0] * self.base_scales[1]
        self.mult_inverse = [multiplicative_inverse(self.base_scales[1], self.base_scales[0]), multiplicative_inverse(self.base_scales[0], self.base_scales[1])]

    @classmethod
    def of_scene(cls, scene):
        d = scene.desc
        perms = np.ctypeslib.as_array(d.sampler.perms, (int(d.sampler.n_perms),))
        return cls(d.film.xres, d.film.yres, d.sampler.sample_at_center, perms.tolist())

    def check_desc(self, desc):
        """what this file derived against the description's fields"""
        s = desc.sampler
        assert list(s.base_scales) == self.base_scales and list(s.base_exponents) == self.base_exponents, (list(s.base_scales), list(s.base_exponents))
        assert int(s.sample_stride) == self.sample_stride and list(s.mult_inverse) == self.mult_inverse, (int(s.sample_stride), list(s.mult_inverse))
        assert bool(s.sample_at_center) == self.sample_at_center and int(s.n_perms) == len(self.perms)

    def check_perms(self):
        """every base's slice of the table is a permutation of its digits"""
        for b, start in zip(PRIMES, PRIME_SUMS):
            assert sorted(self.perms[start:start + b]) == list(range(b)), b

    def pixel_offset(self, px, py):
        if self.sample_stride <= 1: return 0
        pm = (px % K_MAX_RESOLUTION, py % K_MAX_RESOLUTION)
        offset = 0
        for i, base in enumerate((2, 3)):
            dim_offset = inverse_radical_inverse(base, pm[i], self.base_exponents[1])      # [1] for both: Q24
            offset += dim_offset * (self.sample_stride // self.base_scales[i]) * self.mult_inverse[i]
        return offset % self.sample_stride

    def index(self, px, py, sample_num):
        return self.pixel_offset(px, py) + sample_num * self.sample_stride

    def dim(self, index, d):
        if self.sample_at_center and d in (0, 1): return 0.5
        if d == 0: return radical_inverse(0, index >> self.base_exponents[0])
        if d == 1: return radical_inverse(1, index // self.base_scales[1])
        assert d < PRIME_TABLE_SIZE
        return scrambled_radical_inverse(d, index, self.perms[PRIME_SUMS[d]:PRIME_SUMS[d] + PRIMES[d]])

    def values(self, pixels, sample_nums, first, count):
        """Renderer.sampler_values' answer: index (n,) uint64, v1 (n, count), v2 (n, count, 2)"""
        n = len(sample_nums)
        index = np.zeros(n, np.uint64); v = np.zeros((n, count + 1))
        perm = {d: self.perms[PRIME_SUMS[d]:PRIME_SUMS[d] + PRIMES[d]] for d in range(max(first, 2), first + count + 1)}
        for i, ((px, py), s) in enumerate(zip(pixels, sample_nums)):
            ix = self.index(int(px), int(py), int(s))
            index[i] = ix
            for k in range(count + 1):
                d = first + k
                v[i, k] = self.dim(ix, d) if d < 2 else scrambled_radical_inverse(d, ix, perm[d])
        return index, v[:, :count].copy(), np.stack([v[:, :count], v[:, 1:]], -1)
