"""CPU: the one element-wise bound of tests/test_hip_edges.py that does not follow from the GEMM arithmetic -- BatchNorm's dx over one or two rows, where the
result cancels to (almost) nothing -- is confirmed here the way such a bound has to be: a float32 evaluation of the float64 reference, on the very inputs of
the GPU test, stays inside it (with room to spare), so an f32 kernel that evaluates the same formula can meet it."""
import pytest
import torch

import test_hip_edges as E


@pytest.mark.parametrize("rows", [1, 2])
@pytest.mark.parametrize("Cc", [4, 1024])
def test_bn_dx_small_rows_bound_holds_for_a_float32_evaluation(rows, Cc):
    x, gam, bet, dy, pre, _, dx64 = E.bn_case(rows, Cc)
    dx32 = E.bn_case(rows, Cc, torch.float32)[-1]
    far = (pre.abs() > 1e-5).double()
    err, bound = float(((dx32.double() - dx64) * far).abs().max()), E.bn_dx_small_rows_bound(x, gam, dy)
    assert bound > 0 and err < 0.1 * bound, (err, bound)      # a tenth: a kernel's other order of summation has room
