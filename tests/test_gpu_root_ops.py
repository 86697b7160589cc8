"""GPU: the root operators of csrc/lz_ops.hip -- lz_project_policy_logits_fast, lz_root_pack_rows / _plan / _fill,
lz_root_finalize_from_visits, lz_finalize_trajectory_inplace -- called through the C ABI with the inputs of
tests/root_ops_cases.py and held to the restatements of tests/root_ops_ref.py (which tests/test_root_ops_ref_cpu.py anchors
on the reference's golden values, and runs the host build against).  tests/root_ops_check.py holds the checks.

Every output carries 8 sentinel guard rows on both sides (0xA5 bytes, a NaN with a marked payload); they, and every row the
contract leaves alone, must come back bit for bit.  Integers, masks, masked_logits and everything copied: bit for bit.
Pack priors: (count + 2) * 2^-24 relative.  root_value: (M + 2) * 2^-24 * (sum|w| / max(sum v, 1)) * (1 + sum v / max(sum v, 1)).
Projection probabilities and the finalize policy: 4 x the float32 oracle's own distance from the float64 restatement (per
exponent 1 / T for the policy), never more than the 1e-6 / 1e-5 of tests/test_gpu_ops.py.  Sampled picks: exact -- every
uniform sits in the middle of an interval wider than 1e-3 of the row's total."""
import numpy as np
import pytest
import torch

from tests import root_ops_cases as K
from tests import root_ops_check as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from liuzhou_amd import _lib
    return X.Build(_lib, "cuda:0")


@pytest.mark.parametrize("T", K.PROJECT_T)
def test_projection_equals_the_restatement(gpu, T):
    """auxiliary_dim 0, 1, 4, 40; B = 1, 3 leave waves of the workgroup idle, 5 and 257 end inside one."""
    worst = max(X.check_project(gpu, K.project_case(T, B)) for B in K.PROJECT_B)
    print(f"T={T}: kernel's worst probability error {worst:.3e}, bound and oracle's own {X.project_bound()}")


@pytest.mark.parametrize("B", K.PACK_B)
def test_pack_rows_plan_and_fill_equal_the_restatement(gpu, B):
    """T = 220, 217, 64, 65 at cap 80 and 72; counts 0, 1, 64, 65 and exactly cap; all rows terminal (R = 0, N = 0 and
    NULL outputs), first and last row terminal; a row under the 1e-8 clamp (exact), a row of zeros, negative metadata."""
    worst = max(X.check_pack_chain(gpu, c)[1] for c in K.pack_cases() if c["B"] == B)
    print(f"B={B}: kernel's worst prior error {worst:.3f} x bound")


@pytest.mark.parametrize("B", K.PLAN_B)
def test_pack_plan_scans_every_batch_size(gpu, B):
    """B > 1024: every thread of the one workgroup scans several rows; runs of terminal rows cross the threads' and the
    waves' chunk boundaries."""
    for c in K.plan_cases():
        if c["B"] == B:
            X.check_pack_plan(gpu, c["counts"], f"B={B} {c['pattern']}")


@pytest.mark.parametrize("sampled", (False, True), ids=("argmax", "sampled"))
@pytest.mark.parametrize("M", K.FIN_M)
def test_finalize_equals_the_restatement(gpu, M, sampled):
    """M <= 64, <= 128, <= 256 are three instances of the kernel; R = 1, 4, 5, 130 with B > R and a root selection with
    gaps; `uniforms` NULL (argmax) and given (every pick exact)."""
    worst, rv = {}, 0.0
    for R in K.FIN_R:
        _, w, ratio = X.check_finalize(gpu, K.finalize_case(M, R), sampled)
        rv = max(rv, ratio)
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"M={M}: kernel's worst policy error per 1/T {worst}, bounds and oracle's own {X.finalize_bounds()}, root_value {rv:.3f} x bound")


@pytest.mark.parametrize("M", (35, 128, 256))
def test_finalize_twice_gives_the_same_bits(gpu, M):
    """policy_dense is built with atomics: with distinct columns the result cannot depend on their order; a root whose row
    scatters two slots to one column may differ by the roundings of its float32 additions (two per run and extra slot)."""
    c = K.finalize_case(M, 130)
    a, b = X.run_finalize(gpu, c, True), X.run_finalize(gpu, c, True)
    for k in X.FIN_OUT[1:]:
        X.assert_bits(a[k], b[k], f"M={M} {k}")
    valid = c["valid"] != 0
    dup = np.zeros(c["B"], bool)
    for r in range(c["R"]):
        cols = c["lidx"][r][valid[r] & (c["lidx"][r] >= 0) & (c["lidx"][r] < c["T"])]
        dup[c["roots"][r]] = np.unique(cols).size < cols.size
    assert dup.any() and not dup.all()
    X.assert_bits(a["policy"][~dup], b["policy"][~dup], f"M={M} policy_dense of the roots with distinct columns")
    diff = np.abs(a["policy"][dup].astype(np.float64) - b["policy"][dup])
    assert (np.nan_to_num(diff) <= 4 * X.Rf.F32_EPS * np.abs(np.nan_to_num(a["policy"][dup]))).all()


def test_argmax_takes_the_overflowed_action_not_slot_0(gpu):
    """visits^(1/T) overflows float32 from about 7132 visits at T = 0.1 (and from 2 at the temperature clamp): the
    reference's policy is NaN there and 0 elsewhere, and torch's max takes the first NaN.  Slot 0 is padding in row 0."""
    c = K.overflow_pin_case()
    got, _, _ = X.check_finalize(gpu, c, False)
    assert got["chosen_index"].tolist() == [-1, 9, 11] and got["chosen_valid"].tolist() == [0, 1, 1]


def test_root_value_is_written_for_a_row_without_valid_action(gpu):
    got, _, _ = X.check_finalize(gpu, K.no_valid_pin_case(), False)
    assert got["root_value"].tolist() == [0.5, -0.25, 2.0] and got["chosen_valid"].tolist() == [0, 0, 1, 0]


@pytest.mark.parametrize("max_steps", K.TRAJ_STEPS)
def test_finalize_trajectory_equals_the_restatement(gpu, max_steps):
    """F = 1, 4, 5, 300 finished slots over G = 1, 12, 300 games; games of 0, 1, 64, 65, max_steps and max_steps + 3 steps
    (the lanes' stride iterates, the count is clamped); slots -1 and G; results -1, 0, +1, -0.0; counts_out is added to."""
    for c in K.traj_cases():
        if c["max_steps"] == max_steps:
            X.check_traj(gpu, c)
