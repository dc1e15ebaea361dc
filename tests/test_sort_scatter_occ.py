"""The low-LDS radix scatter (k_rs8_scatter_occ) against numpy's stable
argsort and against the LDS scatter it replaces.

A stable sort has exactly one correct output, so every comparison is exact:
for each case the new variant's sorted keys, index payload and second
payload equal (1) the numpy reference and (2) the "lds" variant's outputs.

Shapes are the smallest at which the kernel can go wrong: one item, the
wave (64) and block (256) edges, the 4096-item tile edge, three tiles plus
one item, and 25 tiles with a ragged last tile and a partly empty last wave.
`base_shift + bits` never exceeds 32 (the keys are 32 bits wide), so the
21-bit, three-pass cases run at shift 0 only.
"""
import functools

import numpy as np
import pytest

from windflow_amd import _core

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 12_289, 100_003]
BITS = [5, 8, 9, 15, 16, 21]
SHIFTS = [0, 16]


def _field(dist, n, bits, seed):
    """The sorted-on key field (values below 2**bits) of a distribution."""
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.uint64)
    top = (1 << bits) - 1
    if dist == "uniform":
        f = rng.integers(0, 1 << bits, size=n, dtype=np.uint64)
    elif dist == "equal":
        # one digit owns the whole tile: the per-wave counter reaches 1024
        # and the run length 4096
        f = np.full(n, top - 2, dtype=np.uint64)
    elif dist == "two":
        f = np.where(i % 2 == 0, np.uint64(top), np.uint64(1))
    elif dist == "mod256":
        f = i % 256  # every lane of a round a distinct digit
    elif dist == "div64":
        f = (i // 64) % 256  # every lane of a round the same digit
    elif dist == "descending":
        f = (np.uint64(top) - (i % np.uint64(top + 1)))
    elif dist == "topdigit":
        # low byte zero: pass 0 is the identity permutation
        hi = max(bits - 8, 1)
        f = rng.integers(0, 1 << hi, size=n, dtype=np.uint64) << np.uint64(8)
    else:
        raise ValueError(dist)
    return (f & np.uint64(top)).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _case(dist, n, bits, base_shift, seed=5):
    """(keys, order) for a case; computed once and shared, never modified."""
    f = _field(dist, n, bits, seed)
    keys = f << np.uint32(base_shift)
    if base_shift:
        # low bits ride along: they must come back attached to their keys
        # and must not influence the order
        rng = np.random.default_rng(seed + 1)
        keys = keys | rng.integers(0, 1 << base_shift, size=n, dtype=np.uint32)
    keys = keys.astype(np.uint32)
    order = np.argsort((keys >> np.uint32(base_shift)) & np.uint32((1 << bits) - 1),
                       kind="stable")
    keys.setflags(write=False)
    order.setflags(write=False)
    return keys, order


def _vals2(n):
    return (np.arange(n, dtype=np.uint32) * np.uint32(2654435761)) ^ np.uint32(0xA5A5A5A5)


def _check(keys, order, bits, base_shift, implicit_iota=True, prehist=False,
           carry=False, variants=("occ", "lds")):
    n = len(keys)
    v2 = _vals2(n) if carry else None
    got = {}
    for var in variants:
        ks, vs, ws = _core.debug_sort_pairs2(
            keys, bits, base_shift=base_shift, implicit_iota=implicit_iota,
            prehist=prehist, vals2=v2, variant=var)
        got[var] = (ks, vs, ws)
        tag = f"variant={var!r}"
        assert np.array_equal(ks, keys[order]), tag
        assert np.array_equal(vs, order.astype(np.uint32)), tag
        if carry:
            assert np.array_equal(ws, v2[order]), tag
        else:
            assert ws is None, tag
    base = got[variants[0]]
    for var in variants[1:]:
        assert np.array_equal(base[0], got[var][0])
        assert np.array_equal(base[1], got[var][1])
        if carry:
            assert np.array_equal(base[2], got[var][2])


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_pass_counts(n, bits):
    for base_shift in SHIFTS:
        if base_shift + bits > 32:
            continue
        keys, order = _case("uniform", n, bits, base_shift)
        _check(keys, order, bits, base_shift)


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_pass_counts_second_payload(n, bits):
    for base_shift in SHIFTS:
        if base_shift + bits > 32:
            continue
        keys, order = _case("uniform", n, bits, base_shift)
        _check(keys, order, bits, base_shift, carry=True)


@pytest.mark.parametrize("carry", [False, True])
@pytest.mark.parametrize("bits,base_shift", [(8, 0), (9, 0), (15, 16), (16, 16),
                                             (21, 0)])
@pytest.mark.parametrize("dist", ["equal", "two", "mod256", "div64",
                                  "descending", "topdigit"])
def test_key_distributions(dist, bits, base_shift, carry):
    for n in (4096, 4097, 12_289, 100_003):
        keys, order = _case(dist, n, bits, base_shift)
        _check(keys, order, bits, base_shift, carry=carry)


@pytest.mark.parametrize("prehist", [False, True])
@pytest.mark.parametrize("carry", [False, True])
@pytest.mark.parametrize("implicit_iota", [True, False])
@pytest.mark.parametrize("bits,base_shift", [(5, 0), (9, 0), (15, 0), (15, 16),
                                             (16, 16), (21, 0)])
def test_option_combinations(bits, base_shift, implicit_iota, carry, prehist):
    # dense keys below 2**bits, as the fused dense-key kernel requires
    for n in (1, 65, 4097, 12_289, 100_003):
        keys, order = _case("uniform", n, bits, base_shift)
        _check(keys, order, bits, base_shift, implicit_iota=implicit_iota,
               prehist=prehist, carry=carry, variants=("occ", "lds", ""))


@pytest.mark.parametrize("carry", [False, True])
@pytest.mark.parametrize("prehist", [False, True])
def test_back_to_back_calls_share_buffers(prehist, carry):
    """Two sorts in a row on different data of different n.  Both sizes
    round to the same arena buffer sizes (key arrays and histogram scratch),
    so the second call runs on the first call's leftovers."""
    first = [(12_300, "equal"), (4160, "mod256")]
    second = [(12_289, "uniform"), (4097, "descending")]
    for (n1, d1), (n2, d2) in zip(first, second):
        for bits, base_shift in ((15, 16), (9, 0)):
            k1, o1 = _case(d1, n1, bits, base_shift)
            k2, o2 = _case(d2, n2, bits, base_shift)
            for var in ("occ", "lds"):
                _check(k1, o1, bits, base_shift, prehist=prehist, carry=carry,
                       variants=(var,))
                _check(k2, o2, bits, base_shift, prehist=prehist, carry=carry,
                       variants=(var,))


def test_unknown_variant_is_an_error():
    keys, _ = _case("uniform", 65, 9, 0)
    with pytest.raises(RuntimeError):
        _core.debug_sort_pairs2(keys, 9, variant="nope")
