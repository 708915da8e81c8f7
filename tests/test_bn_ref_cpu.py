"""CPU self-check of the per-view BatchNorm reference (tests/bn_ref.py): the closed forms against torch autograd through the
oracle's batch_norm_train_grouped, both in float64, at the geometries of the kernel sweep (tests/test_gpu_train_lp.py)."""
import pytest
import torch

import bn_ref
from oracle import backbone as OB

# (N, V, h, w, c) of the sweep's small cases A..F and H
GEOMETRIES = [(3, 4, 7, 7, 80), (4, 3, 10, 9, 200), (24, 4, 1, 1, 64), (40, 2, 2, 2, 72), (6, 5, 3, 3, 136),
              (3, 4, 7, 7, 6), (80, 4, 1, 1, 64)]


def rel(a, d):
    return float((a.double() - d.double()).abs().max()) / max(float(d.double().abs().max()), 1e-300)


@pytest.mark.parametrize("with_gamma", [False, True])
@pytest.mark.parametrize("N,V,h,w,c", GEOMETRIES)
def test_closed_forms_equal_autograd_through_the_oracle(N, V, h, w, c, with_gamma):
    g = torch.Generator().manual_seed(N * 1000 + c)
    nb = N * V
    z = (torch.randn(nb, h, w, c, generator=g, dtype=torch.float64) * 2 + 0.5).requires_grad_(True)
    beta = torch.randn(c, generator=g, dtype=torch.float64).requires_grad_(True)
    gamma = (torch.rand(c, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True) if with_gamma else None
    dy = torch.randn(nb, h, w, c, generator=g, dtype=torch.float64)
    groups = [b % V for b in range(nb)]
    y_lin, mean, var = OB.batch_norm_train_grouped(z, beta, gamma, 1e-3, groups)
    mask = (y_lin > 0).detach()
    (y_lin * mask).backward(dy)

    gm = gamma.detach() if with_gamma else None
    f = bn_ref.forward(z.detach(), V, beta.detach(), gm, 1e-3)
    assert rel(f["mean"], mean.detach()) <= 1e-12 and rel(f["var"], var.detach()) <= 1e-12
    assert rel(f["y"], torch.relu(y_lin.detach())) <= 1e-12
    assert torch.equal(f["y"] > 0, mask)
    b = bn_ref.backward(z.detach(), dy, mask, V, gm, 1e-3)
    assert rel(b["dz"], z.grad) <= 1e-12
    assert rel(b["dbeta"], beta.grad) <= 1e-12
    if with_gamma:
        assert rel(b["dgamma"], gamma.grad) <= 1e-12
    # the raw totals, view by view (image b is view b % V)
    zd = z.detach()
    for v in range(V):
        zv, gv = zd[v::V], (dy * mask)[v::V]
        assert rel(f["sum_z"][v], zv.sum((0, 1, 2))) <= 1e-12
        assert rel(f["sum_z2"][v], (zv * zv).sum((0, 1, 2))) <= 1e-12
        zh = (zv - mean.detach()[v]) * torch.rsqrt(var.detach()[v] + 1e-3)
        assert rel(b["sum_g"][v], gv.sum((0, 1, 2))) <= 1e-12
        assert rel(b["sum_gzh"][v], (gv * zh).sum((0, 1, 2))) <= 1e-12
    assert rel(b["dbeta"], b["sum_g"].sum(0)) <= 1e-12 and rel(b["dgamma"], b["sum_gzh"].sum(0)) <= 1e-12


def test_recomputed_mask_follows_the_view_of_each_image():
    V, nb, c = 3, 6, 4
    z = torch.ones(nb, 2, 2, c)
    scale = torch.ones(V, c)
    shift = -torch.arange(V, dtype=torch.float32)[:, None].expand(V, c)     # view 0: 1 > 0; view 1: 0; view 2: -1
    mask = bn_ref.mask_from_z(z, V, scale, shift)
    assert mask.shape == z.shape and mask.dtype == torch.bool
    assert [bool(mask[b].all()) for b in range(nb)] == [b % V == 0 for b in range(nb)]
    assert [bool(mask[b].any()) for b in range(nb)] == [b % V == 0 for b in range(nb)]
    # one rounding of the exact value (a fused multiply-add): (1 + 2^-23)(1 - 2^-24) - 1 = 2^-24 - 2^-47 > 0, though the
    # product rounded to float32 on its own is 1
    tiny = bn_ref.mask_from_z(torch.full((1, 1, 1), 1.0 + 2.0 ** -23), 1, torch.tensor([[1.0 - 2.0 ** -24]]),
                              torch.tensor([[-1.0]]))
    assert bool(tiny.all())
