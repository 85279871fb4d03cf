"""GPU parity of the totals decoder's sign-bit check step (projectultra_amd/csrc/ldpc_totals_kernel.h, kSignBits): the channel
values are canonicalised where they are staged (-0.0 -> +0.0, NaN -> +inf) and the loop then takes the sign bit for `x < 0`.
Inputs made to catch the two values where the sign bit and `x < 0` differ, and totals that cancel to exactly zero: all six
rates (the low-rate instances keep the compare form and must agree too), iteration limits 0 / 1 / 50 / 200, the screen off and
forced, the fused deinterleaver.  Every case is compared with the oracle bit for bit: bytes, iterations, success."""
import os

import numpy as np
import pytest

from _util import noisy_codewords

pytestmark = pytest.mark.gpu
RATES = [0, 1, 2, 3, 4, 5]
SIG = {0: [1.7, 2.2], 1: [1.0, 1.3], 2: [1.0, 1.3], 3: [0.75, 0.9], 4: [0.6, 0.75], 5: [0.5, 0.6]}
# +-0, NaN of both signs with several payloads (quiet and signalling), +-inf, +-FLT_MAX, +-the smallest denormal
SPECIALS = np.array([0x00000000, 0x80000000, 0x7FC00000, 0xFFC00000, 0x7FA00001, 0xFFC12345, 0x7F800001, 0xFF800001,
                     0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x80000001], dtype=np.uint32)
# small values whose sums and differences cancel to exactly zero (llr = 0.75 m against a message -0.75 m)
SMALL = np.array([0.75, -0.75, 0.5, -0.5, 0.0, -0.0, 1.5, -1.5], dtype=np.float32)


@pytest.fixture
def screen(request):
    old = os.environ.get("ULTRA_HIP_LDPC_SCREEN")
    os.environ["ULTRA_HIP_LDPC_SCREEN"] = request.param     # read by ultra_hip_create
    yield request.param
    if old is None:
        os.environ.pop("ULTRA_HIP_LDPC_SCREEN", None)
    else:
        os.environ["ULTRA_HIP_LDPC_SCREEN"] = old


def _decoder(rate, max_iter=50):
    from projectultra_amd import CodeRate, LDPCDecoder
    d = LDPCDecoder(CodeRate(rate))
    if max_iter != 50:
        d.setMaxIterations(max_iter)
    return d


def _same(r, want, what):
    ob, oi, ook = want[:3]
    assert np.array_equal(r["iters"], oi), (what, np.flatnonzero(r["iters"] != oi)[:8])
    assert np.array_equal(r["ok"], ook), what
    assert np.array_equal(r["bytes"], ob), (what, np.flatnonzero((r["bytes"] != ob).any(axis=1))[:8])


def _cases(oracle, rate, seed):
    """noisy codewords; the same with specials sprinkled in; codewords of one special value each; codewords of random specials;
    small-alphabet codewords; a valid codeword's signs carried by -0.0 / +0.0 and by NaNs of either sign"""
    rng = np.random.default_rng(seed)
    noisy, _ = noisy_codewords(oracle, rate, 96, SIG[rate], seed=seed)
    n = noisy.shape[1]
    sprinkled = noisy.copy()
    mask = rng.random(sprinkled.shape) < 0.125
    sprinkled[mask] = SPECIALS[rng.integers(0, len(SPECIALS), mask.sum())].view(np.float32)
    uniform = np.repeat(SPECIALS.view(np.float32)[:, None], n, axis=1)
    mixed = SPECIALS[rng.integers(0, len(SPECIALS), (32, n))].view(np.float32)
    small = SMALL[rng.integers(0, len(SMALL), (64, n))]
    signs = np.signbit(noisy[:16])
    zeros = np.where(signs, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    nans = np.where(signs, np.uint32(0xFFC00001), np.uint32(0x7FC00001)).astype(np.uint32).view(np.float32)
    return np.ascontiguousarray(np.concatenate([noisy, sprinkled, uniform, mixed, small, zeros, nans]).astype(np.float32))


@pytest.mark.parametrize("screen", ["0", "2"], indirect=True)
@pytest.mark.parametrize("rate", RATES)
def test_signbits_special_values(oracle, screen, rate):
    llr = _cases(oracle, rate, 300 + rate)
    _same(_decoder(rate).decode_batch(llr), oracle.ldpc_decode_batch(rate, llr), (rate, screen))


@pytest.mark.parametrize("screen", ["0", "2"], indirect=True)
@pytest.mark.parametrize("max_iter", [0, 1, 200])
def test_signbits_iteration_limits(oracle, screen, max_iter):
    for rate in RATES:
        llr = _cases(oracle, rate, 400 + rate)
        _same(_decoder(rate, max_iter).decode_batch(llr), oracle.ldpc_decode_batch(rate, llr, max_iters=max_iter),
              (rate, max_iter, screen))


@pytest.mark.parametrize("screen", ["0", "2"], indirect=True)
@pytest.mark.parametrize("rate,bps", [(4, 4), (3, 2), (5, 6)])
def test_signbits_fused_deinterleaver(oracle, screen, rate, bps):
    from projectultra_amd import ChannelInterleaver
    llr = _cases(oracle, rate, 500 + rate)
    want = oracle.ldpc_decode_batch(rate, llr)
    d = _decoder(rate)
    il = ChannelInterleaver(bps)
    d.setDeinterleave(bps)
    _same(d.decode_batch(np.stack([il.interleave(r) for r in llr])), want, (rate, bps, screen))
