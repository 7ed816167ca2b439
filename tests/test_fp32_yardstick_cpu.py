"""The inputs of test_fp32_equivalence_gpu.py discriminate: on the CPU, with the oracle's own products cut to bf16 planes
(tests/precision_yardstick.py), three planes per operand stay inside the fp32 bound of every output group and two planes miss
it by more than a factor of two.  A GPU test that holds a kernel to that bound therefore cannot pass with a two-plane kernel."""
import pytest

from tests import precision_yardstick as py


@pytest.mark.parametrize("case", ["policy", "prior", "vposer"])
def test_bound_separates_three_planes_from_two(case):
    c = {"policy": py.policy_case, "prior": py.prior_case, "vposer": py.vposer_case}[case]()
    e3, e2 = c.error(c.emulated(3)), c.error(c.emulated(2))
    py.emit(py.table(c, f"{case}: oracle with truncated operands (CPU)", {"3 planes": e3, "2 planes": e2}), env="EGX_F32_CPU_TABLE")
    assert set(e3) == set(c.groups) == set(e2)
    for g in c.groups:
        assert e3[g] <= c.bound(g), (g, e3[g], c.bound(g))
        assert e2[g] > 2 * c.bound(g), (g, e2[g], c.bound(g))


def test_planes_are_the_bf16_split():
    """planes(x, k) keeps 8, 16, 24 significant bits: k = 3 reproduces fp32 exactly, k = 1 is bf16 rounding."""
    import torch
    x = torch.randn(4096, generator=torch.Generator().manual_seed(0)) * torch.logspace(-20, 20, 4096)
    assert torch.equal(py.planes(x, 3), x.double())
    assert torch.equal(py.planes(x, 1), x.bfloat16().double())
    e2 = ((py.planes(x, 2) - x.double()).abs() / x.double().abs()).max()
    assert 2.0 ** -18 < float(e2) <= 2.0 ** -16   # each plane (8 significant bits) rounds its residual to 2^-8 relative


def test_truncation_is_restored():
    from oracle import nets
    lin, gru = nets.linear, nets.gru_cell
    with pytest.raises(RuntimeError):
        with py.truncated_products(2):
            assert nets.linear is not lin
            raise RuntimeError
    assert nets.linear is lin and nets.gru_cell is gru
