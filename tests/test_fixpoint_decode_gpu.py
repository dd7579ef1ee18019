"""The step kernels' fixed-point decode with a wave-uniform fast path (from_fix_wave,
csrc/include/convnet_dev.h): when q >> 24 of every value a wave decodes fits an int32, the high
part converts with a 32-bit conversion, else the wave takes from_fix as it stands.  A test-only
kernel (fix_decode, csrc/kernels/diag.hip) evaluates both on the same int64 inputs the way the
backward's h phase does -- 4 consecutive values per thread, so 256 per wave -- and the results
must agree bit for bit, for both scales (2^-32 dense-1 sums, 2^-40 conv gradient).

The inputs are laid out so that some waves are all fast path, some all fallback and some
mixed; the edge values sit in each kind."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WAVE = 256  # values per wave: 64 lanes x 4
I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1

# |q| < 2^55: q >> 24 fits an int32 (the fast path's domain), and the rest
_NARROW = [0, 1, -1, 2 ** 24 - 1, -(2 ** 24 - 1), 2 ** 24, -(2 ** 24), 2 ** 47, -(2 ** 47),
           2 ** 48 + 1, 2 ** 48 - 1, -(2 ** 48 + 1), -(2 ** 48 - 1), 2 ** 55 - 1, -(2 ** 55 - 1), -(2 ** 55)]
_WIDE = [2 ** 55, 2 ** 62, -(2 ** 62), I64_MIN, I64_MAX, -(2 ** 55) - 1, 2 ** 55 + 1]


def _narrow(q):
    return np.isin(q >> 55, (0, -1))


def _random(rng, n, lo_bits, hi_bits):
    """n values of every magnitude: bit length uniform in [lo_bits, hi_bits], random sign"""
    bits = rng.integers(lo_bits, hi_bits + 1, n)
    mag = rng.integers(0, 2 ** 62, n, dtype=np.int64) | (np.int64(1) << 62)  # top bit set, 63 bits
    mag = np.where(bits == 0, 0, mag >> np.maximum(63 - bits, 0).astype(np.int64))
    return np.where(rng.integers(0, 2, n) == 1, -mag, mag).astype(np.int64)


def _inputs():
    rng = np.random.default_rng(1234)
    fast = _random(rng, 8 * WAVE, 0, 55)       # bit length <= 55: |q| < 2^55
    fast[rng.choice(len(fast), len(_NARROW), replace=False)] = _NARROW
    slow = _random(rng, 4 * WAVE, 56, 63)      # every value needs the fallback
    slow[rng.choice(len(slow), len(_WIDE), replace=False)] = _WIDE
    mixed = _random(rng, 8 * WAVE, 0, 63)
    both = np.array(_NARROW + _WIDE, dtype=np.int64)
    mixed[rng.choice(len(mixed), len(both), replace=False)] = both
    # waves of narrow values with a single wide one, in the first / last lane and in between
    lone = _random(rng, 3 * WAVE, 0, 55)
    lone[0], lone[WAVE + 131], lone[3 * WAVE - 1] = 2 ** 55, I64_MIN, -(2 ** 60)
    q = np.concatenate([fast, slow, mixed, lone])
    kinds = _narrow(q).reshape(-1, WAVE)
    n_fast, n_slow = int(kinds.all(1).sum()), int((~kinds).all(1).sum())
    assert n_fast >= 8 and n_slow >= 4 and len(kinds) - n_fast - n_slow >= 8, (n_fast, n_slow, len(kinds))
    assert _narrow(fast).all() and not _narrow(slow).any()
    return q


@pytest.mark.parametrize("scale", [0, 1], ids=["HINV", "CINV"])
def test_wave_decode_equals_from_fix_bitwise(scale):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from distributed_amd.native import require_C

    qh = _inputs()
    q = torch.from_numpy(qh).cuda()
    fast = torch.full((len(qh),), float("nan"), dtype=torch.float32, device="cuda")
    ref = torch.full_like(fast, float("nan"))
    require_C().fix_decode(q.data_ptr(), fast.data_ptr(), ref.data_ptr(), len(qh), scale, 0)
    torch.cuda.synchronize()
    f, r = fast.cpu().numpy(), ref.cpu().numpy()
    bad = np.flatnonzero(f.view(np.int32) != r.view(np.int32))
    assert bad.size == 0, [(int(qh[i]), float(f[i]), float(r[i])) for i in bad[:8]]
    assert np.isfinite(r).all()
    # and from_fix itself is the correctly rounded q * 2^-s where its comment says so: |q| < 2^48
    # is exact in a double, the product by a power of two too, and double -> float rounds once
    small = np.abs(qh.astype(np.float64)) < 2.0 ** 48
    inv = 2.0 ** -32 if scale == 0 else 2.0 ** -40
    want = (qh[small].astype(np.float64) * inv).astype(np.float32)
    assert np.array_equal(r[small].view(np.int32), want.view(np.int32))
