"""Which kernel serves which geometry, asked of the library on the host (no GPU): the template families of
csrc/conv_pwbwd.hip and csrc/irdw.hip are instantiated per tile count and picked at run time through
nasseg_conv_pw_bwd_kernel_id / nasseg_irdw_config - the table the launches themselves go through.

* What functional._irdw_ok admits (InvertedResidual's expansion never stored: the forward drops z1) must have a kernel
  that rebuilds z1 in every backward that needs it.  A geometry admitted without one either read a null pointer
  (K <= 16, 96 < N <= 144) or failed in the middle of the step (N > 144 at stride 2).
* Every instantiation must be launched by a case of the exact-arithmetic GPU tests (tests/test_hip_exact.py): an
  instantiation added without a case fails here, and so does a case removed that was the only one to reach a kernel."""
import collections

import pytest
import torch

from test_hip_exact import HUGE, IRDW_CASES, PW_BWD_CASES, knobs, pw_bwd_kernel_ids


def F():
    from nas_segm_amd import functional

    return functional


# ---------------------------------------------------------------------------------------------------------------
# the gate of the "expansion never stored" form admits nothing that a kernel does not serve
# ---------------------------------------------------------------------------------------------------------------
_Op = collections.namedtuple("_Op", "kind stride pad dil has_bn act training")
# a map below the small-map slab rule of the pointwise backward (fewer than 256 slabs of four tiles) and one of 2^18 pixels
GATE_MAPS = [(2, 48, 64), (1, 512, 512)]


def _admitted(f, B, H, W, K, N, stride):
    """functional._irdw_ok itself over a pointwise conv K -> N + BatchNorm + ReLU6 and a 3x3 depthwise conv + BatchNorm
    in a training step with both gradients wanted (shapes only: tensors on the meta device)"""
    ops = [_Op("dense", 1, 0, 1, True, 2, True), _Op("dw", stride, 1, 1, True, 2, True)]
    weights = [torch.empty(N, K, 1, 1, device="meta"), torch.empty(N, 1, 3, 3, device="meta")]
    cur = torch.empty(B, K, H, W, device="meta")
    return f._irdw_ok(ops, 0, weights, cur, None, True, True, True)


@pytest.mark.parametrize("B,H,W", GATE_MAPS, ids=lambda v: str(v))
def test_the_gate_admits_only_what_a_rebuilding_kernel_serves(B, H, W, monkeypatch):
    f = F()
    monkeypatch.setattr(f, "IRDW", True)
    monkeypatch.setattr(f, "_IRDW_MIN_PIXELS", 0)
    lib = f.lib
    admitted, unserved = 0, []
    for stride in (1, 2):
        for K in range(4, 33, 4):
            for N in range(16, 193, 16):
                if not _admitted(f, B, H, W, K, N, stride):
                    continue
                admitted += 1
                kid = lib.query("nasseg_conv_pw_bwd_kernel_id", B, H, W, K, N, 1)
                ok = 0 <= kid < 10000 and kid % 10 == 1  # (a narrow kernel with its rebuild bit set)
                ok = ok and all(lib.query("nasseg_irdw_config", B, H, W, K, N, stride, bwd) > 0 for bwd in (0, 1))
                ok = ok and all(lib.query("nasseg_irdw_rows", B, H, W, K, N, stride, bwd) > 0 for bwd in (0, 1))
                if not ok:
                    unserved.append((K, N, stride, kid))
    # (the reference network's expansions are among the admitted: the sweep is not vacuous)
    assert admitted >= 40 and _admitted(f, B, H, W, 16, 96, 2) and _admitted(f, B, H, W, 24, 144, 1)
    assert not unserved, "{} admitted geometries (K, N, stride, kernel id) without a kernel: {}".format(
        len(unserved), unserved)


def test_the_gate_follows_the_kernel_table_not_a_channel_bound():
    """the geometries that were admitted without a kernel are refused now, their neighbours with one still admitted;
    and nasseg_conv_pw_bwd_kernel_id never names a z-loading kernel for a call without z"""
    f = F()
    lib = f.lib
    q = lambda K, N, zn: lib.query("nasseg_conv_pw_bwd_kernel_id", 1, 512, 512, K, N, zn)  # noqa: E731
    assert q(16, 128, 1) == -1 and q(16, 144, 1) == -1 and q(8, 112, 1) == -1   # nt = 9, kt = 1: no rebuilding kernel
    assert q(16, 160, 1) == -1 and q(24, 192, 1) == -1 and q(32, 192, 1) == -1  # nt = 12
    assert q(16, 128, 0) == 910 and q(16, 160, 0) == 1210 and q(32, 192, 0) == 1220  # (served with z given)
    assert q(24, 144, 1) == 921 and q(16, 96, 1) == 611 and q(8, 32, 1) == 211
    assert q(224, 64, 0) == 10004 and q(224, 64, 1) == -1 and q(388, 64, 0) == -1 and q(16, 18, 0) == -1
    for K in range(4, 385, 4):
        for N in range(4, 193, 4):
            kid = q(K, N, 1)
            assert kid == -1 or (kid < 10000 and kid % 10 == 1), (K, N, kid)


# ---------------------------------------------------------------------------------------------------------------
# every instantiation is launched by a case of the exact GPU tests
# ---------------------------------------------------------------------------------------------------------------
def _all_pw_bwd_ids(lib):
    ids = set()
    for rz in (0, HUGE):
        with knobs(conv_pw_bwd_rz_min_pixels=rz):
            for K in range(4, 385, 4):
                for N in range(4, 193, 4):
                    for zn in (0, 1):
                        ids.add(lib.query("nasseg_conv_pw_bwd_kernel_id", 2, 8, 16, K, N, zn))
    ids.discard(-1)
    return ids


def test_every_pointwise_backward_instantiation_has_an_exact_case():
    """per id three kernels: with an input prologue (PRO, and DXS where K <= 64: the exact test runs its dx_stats call
    whenever the case has a prologue) and without.  Each case reaches its ids with z loaded, z rebuilt and z == NULL"""
    lib = F().lib
    ids = _all_pw_bwd_ids(lib)
    narrow = {i for i in ids if i < 10000}
    # (the enumeration itself: 16 (nt, kt) that load z, 9 that rebuild it, the wide kernel with 2 .. 6 chunks)
    assert len({i for i in narrow if i % 10 == 0}) >= 16 and len({i for i in narrow if i % 10 == 1}) >= 9
    assert {i - 10000 for i in ids - narrow} >= {2, 3, 4, 5, 6}
    reached = set()
    for geom in PW_BWD_CASES:
        reached |= pw_bwd_kernel_ids(lib, geom)
    missing = sorted({(i, pro) for i in ids for pro in (False, True)} - reached)
    assert not missing, "(kernel id, prologue) without a case in test_hip_exact.PW_BWD_CASES: {}".format(missing)
    # the wide kernel's four waves split N: a case with a single tile of N (three waves idle)
    assert any(g[1][4] <= 16 and i >= 10000 for g in PW_BWD_CASES for i, _ in pw_bwd_kernel_ids(lib, g))


def _irdw_classes(stride, cfg):
    """what distinguishes one launch of irdw_fwd_kernel / irdw_bwd_kernel from another: the instantiation <stride, kt>
    (the prologue is a parameter of the tests), the workgroup size 64 * waves at either stride and tile count of K, and
    whether the grid has a second dimension (groups of channel tiles)"""
    waves, groups, kt = cfg // 1000, cfg // 10 % 100, cfg % 10
    return {("stride, kt", stride, kt), ("waves, stride", waves, stride), ("waves, kt", waves, kt),
            ("waves, several groups", waves, groups > 1)}


def test_every_irdw_launch_shape_has_an_exact_case():
    lib = F().lib
    want = set()
    for B, H, W in GATE_MAPS:
        for stride in (1, 2):
            for K in range(4, 33, 4):
                for C in range(16, 193, 16):
                    cfg = [lib.query("nasseg_irdw_config", B, H, W, K, C, stride, bwd) for bwd in (0, 1)]
                    assert cfg[0] > 0 and cfg[0] == cfg[1], (K, C, stride, cfg)
                    assert all(lib.query("nasseg_irdw_rows", B, H, W, K, C, stride, bwd) > 0 for bwd in (0, 1))
                    want |= _irdw_classes(stride, cfg[0])
    assert {c[1] for c in want if c[0] == "waves, kt"} == {1, 2, 3, 4} and len(want) >= 4 + 8 + 8 + 8
    assert lib.query("nasseg_irdw_config", 1, 16, 16, 36, 96, 1, 0) == 0  # (K > 32: not served)
    assert lib.query("nasseg_irdw_config", 1, 16, 16, 16, 208, 1, 0) == 0  # (C > 192)
    got = set()
    for _, (B, K, C, H, W, stride) in IRDW_CASES:
        cfg = lib.query("nasseg_irdw_config", B, H, W, K, C, stride, 0)
        assert cfg > 0 and cfg == lib.query("nasseg_irdw_config", B, H, W, K, C, stride, 1)
        got |= _irdw_classes(stride, cfg)
    missing = sorted(want - got)
    assert not missing, "launch shapes of csrc/irdw.hip without a case in test_hip_exact.IRDW_CASES: {}".format(missing)
