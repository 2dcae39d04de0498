"""Exact-arithmetic test inputs: small integers and dyadic rationals whose sums no fp32 order can round.

If every term of a sum is an integer multiple of one power-of-two ``unit`` and the sum of the terms' absolute values
stays below 2^24 units, then every product and every partial sum - in ANY order, through FMA, MFMA accumulation,
partial rows or an fp64 finalisation - is exactly representable in fp32, and a kernel must return the mathematical
result: the float64 reference, bit for bit.  With bf16 storage the stored tensor must be the round-to-nearest-even of
that exact value.  Nothing here needs a GPU."""
import torch

LIMIT = float(1 << 24)


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def ints(*shape, lo=-3, hi=3, density=1.0, seed=0, unit=1.0, offset=0.0):
    """fp32 tensor of ``unit * k + offset``, k uniform in lo..hi, zeroed (to ``offset``) with probability
    1 - density.  |lo|, |hi| <= 127 and a power-of-two unit keep every value bf16-representable as long as the offset
    adds no more than one bit (0 or unit / 2)."""
    g = _gen(seed)
    v = torch.randint(int(lo), int(hi) + 1, shape, generator=g).float()
    if density < 1.0:
        v = v * (torch.rand(shape, generator=g) < density).float()
    return v * float(unit) + float(offset)


def halves(*shape, lo=-3, hi=3, seed=0):
    """integers plus 1/2: never 0, never 6, never equal to an integer bound - the no-tie variant of ``ints``"""
    return ints(*shape, lo=lo, hi=hi, seed=seed, offset=0.5)


def pow2(n, lo=-1, hi=1, seed=0, signed=True):
    """n values +- 2^k, k uniform in lo..hi (scales, invstd: multiplying by them is exact)"""
    g = _gen(seed)
    v = torch.pow(2.0, torch.randint(int(lo), int(hi) + 1, (n,), generator=g).float())
    if signed:
        v = v * (torch.randint(0, 2, (n,), generator=g).float() * 2 - 1)
    return v


def bn_vectors(C, seed, tie=True, M=None):
    """(scale, shift, mean, invstd[, sums]) of a BatchNorm with exact arithmetic: scale +-1 | +-2 (so scale * integer
    is an integer), shift a small integer (tie) or integer + 1/2 (no tie: scale * z + shift is never 0 or 6 for an
    integer z), mean a small integer, invstd 1/2 | 1 | 2; sums [2][C] = M * small integers (sums / M is exact for any
    M, and the product with 1 / M is exact when M is a power of two)."""
    scale = pow2(C, 0, 1, seed=seed)
    shift = ints(C, lo=-2, hi=4, seed=seed + 1, offset=0.0 if tie else 0.5)
    mean = ints(C, lo=-1, hi=1, seed=seed + 2)
    invstd = pow2(C, -1, 1, seed=seed + 3, signed=False)
    out = [scale, shift, mean, invstd]
    if M is not None:
        out.append(ints(2 * C, lo=-2, hi=2, seed=seed + 4) * float(M))
    return out


def assert_exactly_summable(op, tensors, unit=1.0, what=""):
    """The precondition, from the reference alone: ``op`` (float64, CPU) over the absolute values of ``tensors`` gives,
    per output element, the sum of the absolute values of its terms; in units of ``unit`` (the common power-of-two
    unit of the op's terms: the product of the inputs' units) it must stay below 2^24.  ``op`` may return one tensor
    or several.  A violation is a mistake in the test's inputs: make them sparser or smaller."""
    outs = op(*[t.detach().double().abs() for t in tensors])
    if isinstance(outs, torch.Tensor):
        outs = [outs]
    worst = 0.0
    for o in outs:
        if o is None or o.numel() == 0:
            continue
        worst = max(worst, float(o.abs().max()) / float(unit))
    assert worst < LIMIT, "{}: sum of |terms| reaches {:.0f} units >= 2^24: inputs are not exactly summable".format(
        what, worst)
    return worst


def assert_stats_summable(z64, unit=1.0, what=""):
    """Statistics rows {sum z, sum z^2} per channel of an NCHW map: the TOTALS of |z| and z^2 over all pixels, in
    units of ``unit`` / ``unit``^2, must stay below 2^24 - that bounds every partition of the pixels into rows."""
    z = z64.detach().double() / float(unit)
    dims = [d for d in range(z.dim()) if d != 1]
    s1, s2 = z.abs().sum(dims), (z * z).sum(dims)
    worst = max(float(s1.max()), float(s2.max()))
    assert worst < LIMIT, "{}: per-channel sum of |z| or z^2 reaches {:.0f} units >= 2^24".format(what, worst)
    return worst


def _first_diff(bad, a, b):
    idx = tuple(int(i) for i in bad.nonzero()[0])
    return idx, a[idx].item(), b[idx].item()


def assert_bitwise(got, ref64, what=""):
    """fp32 ``got``: got.double() == ref64 everywhere; bf16 ``got``: its bits equal those of
    ref64.float().to(bfloat16) (round to nearest even of the exact value).  The sign of a zero is not part of the exact
    value (the float64 reference itself returns either, depending on how it was written; ``==`` does not see it in
    fp32): in the bf16 comparison -0 counts as +0 on both sides."""
    got = got.detach().cpu()
    ref64 = ref64.detach().cpu().double()
    assert tuple(got.shape) == tuple(ref64.shape), "{}: shape {} vs {}".format(what, tuple(got.shape),
                                                                               tuple(ref64.shape))
    if got.numel() == 0:
        return
    if got.dtype == torch.bfloat16:
        want = ref64.float().to(torch.bfloat16)
        zero = torch.zeros((), dtype=torch.bfloat16)
        bad = (torch.where(got == 0, zero, got).contiguous().view(torch.int16)
               != torch.where(want == 0, zero, want).contiguous().view(torch.int16))
        a, b = got.float(), want.float()
    else:
        assert got.dtype in (torch.float32, torch.float64), "{}: dtype {}".format(what, got.dtype)
        a, b = got.double(), ref64
        bad = ~(a == b)  # (a NaN differs from everything)
    n = int(bad.sum())
    if n:
        idx, x, y = _first_diff(bad, a, b)
        raise AssertionError("{}: {} of {} elements differ; first at {}: got {!r}, want {!r}".format(
            what, n, got.numel(), idx, x, y))
