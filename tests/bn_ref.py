"""fp64 reference of the training step's per-view BatchNorm (helper, not collected): train-mode BatchNorm + ReLU with
statistics per view copy (nets/model.py:129-141), forward and backward, restated in plain torch.  Device-agnostic: every
function computes in float64 on the device of its inputs, from the values as they are stored (a bf16 / fp16 / fp32
tensor is widened exactly), so a kernel's result can be held against it at the kernel's own rounding.

    image b belongs to view b % V;  m = (nb / V) * h * w values per (view, channel)
    mean = sum z / m,  var = sum (z - mean)^2 / m (biased),  inv = 1 / sqrt(var + eps)
    scale = gamma * inv,  shift = beta - mean * scale,  y = relu(z * scale + shift)
    g = dy * mask,  zhat = (z - mean) * inv
    dz = gamma * inv * (g - sum g / m - zhat * sum(g zhat) / m),  dbeta = sum_v sum g,  dgamma = sum_v sum g zhat

The ReLU mask is an INPUT of the backward: the kernels define it either by the activation they kept (y > 0, of the stored,
rounded y) or by recomputing float32(z * scale + shift) > 0 from their own fp32 scale / shift (mask_from_z) — taking it
the same way keeps an element at the ReLU edge from counting as a mismatch.
"""
import torch


def _views(t, V):
    """[nb, ..., c] -> float64 [nb / V, V, pixels, c]."""
    nb, c = t.shape[0], t.shape[-1]
    assert nb % V == 0, (nb, V)
    return t.double().reshape(nb // V, V, -1, c)


def _row(s):
    """[V, c] -> [1, V, 1, c]"""
    return s[None, :, None, :]


def _stats(zz, eps):
    m = zz.shape[0] * zz.shape[2]
    mean = zz.sum((0, 2)) / m
    var = ((zz - _row(mean)) ** 2).sum((0, 2)) / m               # two passes: no cancellation
    return m, mean, var, 1.0 / torch.sqrt(var + eps)


def forward(z, V, beta, gamma=None, eps=1e-3, relu=True):
    """z [nb, ..., c], beta / gamma [c] -> dict of float64 tensors: mean, var (biased), inv, scale, shift [V, c]; the raw
    totals sum_z, sum_z2 and sum_abs_z = sum |z| (a bound of every partial sum) [V, c]; y (shape of z)."""
    zz = _views(z, V)
    m, mean, var, inv = _stats(zz, eps)
    scale = inv * gamma.double() if gamma is not None else inv.clone()
    shift = beta.double() - mean * scale
    y = zz * _row(scale) + _row(shift)
    if relu:
        y = y.clamp_min(0.0)
    return {"mean": mean, "var": var, "inv": inv, "scale": scale, "shift": shift, "sum_z": zz.sum((0, 2)),
            "sum_z2": (zz * zz).sum((0, 2)), "sum_abs_z": zz.abs().sum((0, 2)), "y": y.reshape(z.shape)}


def mask_from_z(z, V, scale, shift):
    """The recomputed ReLU mask: float32(z * scale + shift) > 0 with the given [V, c] scale / shift (one rounding of the
    exact value, as the kernels' fused multiply-add)."""
    y = _views(z, V) * _row(scale.double().reshape(V, -1)) + _row(shift.double().reshape(V, -1))
    return (y.float() > 0).reshape(z.shape)


def backward(z, dy, mask, V, gamma=None, eps=1e-3):
    """z, dy, mask [nb, ..., c] -> dict of float64 tensors: dz (shape of z); dbeta, dgamma [c]; the backward totals
    sum_g, sum_gzh and their bounds sum_abs_g = sum |g|, sum_abs_gzh = sum |g zhat| [V, c]."""
    zz = _views(z, V)
    g = _views(dy, V) * _views(mask, V)
    m, mean, var, inv = _stats(zz, eps)
    zh = (zz - _row(mean)) * _row(inv)
    sum_g, sum_gzh = g.sum((0, 2)), (g * zh).sum((0, 2))
    coef = inv * gamma.double() if gamma is not None else inv
    dz = _row(coef) * (g - _row(sum_g) / m - zh * _row(sum_gzh) / m)
    return {"dz": dz.reshape(z.shape), "dbeta": sum_g.sum(0), "dgamma": sum_gzh.sum(0), "sum_g": sum_g,
            "sum_gzh": sum_gzh, "sum_abs_g": g.abs().sum((0, 2)), "sum_abs_gzh": (g * zh).abs().sum((0, 2))}
