"""CPU: the premise the digit cap of k_verify_main_sums rests on (COA_SUMS_CAP,
csrc/coa_sums_tail.h).  A model of halve() (csrc/coa_halve.h) in Python big
integers -- exact Euclid on (8l, k) with the kernel's candidate rule: the three
candidates of every remainder pair once the remainder has at most 136 bits,
d odd, cost = max(bits c, bits d), stop at 124 bits or below -- on 100,000
seeded k.  The kernels run H = (cost + 5) / 4 digits; the cap assumes that about
1.2 % of the items need H >= 34 and that a few need more.  This is a model of
the code, not device output (tools/halve_width_hist.py reads the device's)."""
import random

import ed25519_ref as o

L8 = 8 * o.L


def model_cost(k):
    a, b, ma, mb = L8, k, 0, 1
    best = max(k.bit_length(), 1)

    def consider(c, t):
        nonlocal best
        if t & 1:
            best = min(best, max(c.bit_length(), t.bit_length()))

    while b.bit_length() > 124:
        q, r = divmod(a, b)
        a, b, ma, mb = b, r, mb, ma + q * mb
        if b.bit_length() <= 136:
            consider(b, mb)
            consider(a, ma)
            if (ma ^ mb) & 1:
                consider(a - b, ma + mb)
    return best


def test_model_finds_lattice_vectors():
    """The model's remainders and cofactors are lattice vectors: r == +-t k (mod 8l)."""
    rng = random.Random("coa-halve-tail-lattice")
    for _ in range(50):
        k = rng.randrange(1, o.L)
        a, b, ma, mb, sign = L8, k, 0, 1, 1
        while b.bit_length() > 124:
            q, r = divmod(a, b)
            a, b, ma, mb, sign = b, r, mb, ma + q * mb, -sign
            assert (b - sign * mb * k) % L8 == 0


def test_width_distribution():
    rng = random.Random("coa-halve-tail")
    n = 100_000
    hist = {}
    for _ in range(n):
        H = (model_cost(rng.randrange(1, o.L)) + 5) // 4
        hist[H] = hist.get(H, 0) + 1
    ge34 = sum(c for h, c in hist.items() if h >= 34) / n
    ge35 = sum(c for h, c in hist.items() if h >= 35)
    print(sorted(hist.items()), ge34, ge35)
    assert 0.009 <= ge34 <= 0.016, (ge34, sorted(hist.items()))
    assert ge35 >= 1, sorted(hist.items())
