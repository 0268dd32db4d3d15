"""The checker of the typed-key tests: an independent restatement, in numpy, of the key codec's
table in include/dsort.h ("Key types and order"), and what follows from it.  It shares no code
with the library: dsort.key_encode is what it checks, never what it uses.

    I   w = b
    U   w = b ^ sign_bit
    F   negative floats flip every bit but the sign, the others stay
    descending: ~w

The expected keys of a sort are x[argsort(ref_encode(x), kind="stable")], compared as bits, and
the expected indices that argsort itself.
"""
import numpy as np

KEY_NAMES = ["i32", "u32", "f32", "i64", "u64", "f64"]
KEY_CODE = {k: i for i, k in enumerate(KEY_NAMES)}
NP_TYPE = {"i32": np.int32, "u32": np.uint32, "f32": np.float32,
           "i64": np.int64, "u64": np.uint64, "f64": np.float64}


def width(name):
    return int(name[1:])


def uint_of(name):
    return np.uint32 if width(name) == 32 else np.uint64


def int_of(name):
    return np.int32 if width(name) == 32 else np.int64


def bits(x):
    """The keys as unsigned integers of their width: how results are compared (NaN != NaN)."""
    x = np.ascontiguousarray(x)
    return x.view(np.uint32 if x.dtype.itemsize == 4 else np.uint64)


def ref_encode(x, name, descending=False):
    """The signed words whose order is the order of the typed keys x (any array of the width)."""
    W = width(name)
    U = uint_of(name)
    b = bits(x).copy()
    sign = U(1) << U(W - 1)
    if name[0] == "u":
        w = b ^ sign
    elif name[0] == "f":
        negative = (b & sign) != 0
        w = np.where(negative, b ^ (sign - U(1)), b)
    else:
        w = b
    if descending:
        w = w ^ U((1 << W) - 1)
    return w.astype(U).view(int_of(name))


def ref_order(x, name, descending=False):
    """The stable argsort of x in the typed order: equal keys in ascending position, either way."""
    return np.argsort(ref_encode(x, name, descending), kind="stable")


def from_bits(name, patterns):
    return np.array(patterns, dtype=uint_of(name)).view(NP_TYPE[name])


def curated(name):
    """The curated values of the key type, listed in its ascending order (floats: totalOrder)."""
    W = width(name)
    if name[0] == "i":
        return np.array([-(1 << (W - 1)), -1, 0, 1, (1 << (W - 1)) - 1], dtype=NP_TYPE[name])
    if name[0] == "u":
        return from_bits(name, [0, (1 << (W - 1)) - 1, 1 << (W - 1), (1 << W) - 1])
    mant = 23 if W == 32 else 52
    sign = 1 << (W - 1)
    inf = ((1 << (W - 1 - mant)) - 1) << mant
    one = (((1 << (W - 2 - mant)) - 1) << mant)           # 1.0: the biased exponent 0111..1
    pos = [0,                        # +0
           1,                        # smallest denormal
           1 << mant,                # smallest normal
           one,                      # 1
           inf - 1,                  # max
           inf,                      # +inf
           inf | 1,                  # NaN, payload ...0001
           sign - 1]                 # NaN, all ones
    return from_bits(name, [sign | p for p in reversed(pos)] + pos)


def has_nan_or_negzero(x):
    if x.dtype.kind != "f":
        return False
    return bool(np.isnan(x).any() or ((x == 0) & np.signbit(x)).any())
