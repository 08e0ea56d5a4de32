"""CPU: the float64 restatements of tests/refs64_connector.py are the adjoints they claim to be -- pinned to autograd through the oracle's
pad_or_truncate / adaptive_projection (the reference's glue, oracle/avsr_oracle.py) and to dY.T @ X."""
import pytest
import torch

import refs64_connector as RC
from oracle import avsr_oracle as O

GEOMS = [(9, 7, 3, 9, 12), (9, 7, 3, 9, 5), (9, 7, 3, 9, 20), (9, 7, 3, 9, 1), (9, 0, 0, 9, 4), (0, 7, 0, 7, 11), (12, 7, 2, 9, 8), (1, 0, 0, 1, 6)]


@pytest.mark.parametrize("Ta,Tv,P,L,S", GEOMS)
def test_fuse_pool_bwd_is_autograd_of_the_oracle_glue(Ta, Tv, P, L, S):
    g = torch.Generator().manual_seed(Ta * 100 + S)
    B, D, fs = 2, 8, 0.5 if Ta * Tv == 0 else 0.3
    a = torch.randn(B, Ta, D, generator=g, dtype=torch.float64, requires_grad=True) if Ta else None
    v = torch.randn(B, Tv, D, generator=g, dtype=torch.float64, requires_grad=True) if Tv else None
    pe = torch.randn(B, P, D, generator=g, dtype=torch.float64)
    if a is not None and v is not None:
        x = fs * O.pad_or_truncate(a, L) + (1 - fs) * O.pad_or_truncate(v, L)
    else:
        x = O.pad_or_truncate(a if a is not None else v, L)
    x = torch.cat([pe, x], 1)
    y = O.adaptive_projection(x, S, training=True)
    dx = torch.randn(B, S, D, generator=g, dtype=torch.float64)
    y.backward(dx)
    da, dv = RC.fuse_pool_bwd(dx, Ta, Tv, P, L, fs)
    # the oracle forms the interpolation positions in fp32 (as F.interpolate's caller sees them): 2^-22 relative on a weight
    for got, leaf in ((da, a), (dv, v)):
        if leaf is not None:
            assert float((got - leaf.grad).abs().max()) <= 1e-6 * max(1.0, float(leaf.grad.abs().max()))
    if Ta > L:
        assert float(da[:, L:].abs().max()) == 0.0


@pytest.mark.parametrize("M,N,K", [(1, 8, 8), (65, 64, 24), (200, 16, 40)])
def test_gemm_wgrad_is_the_linear_weight_gradient(M, N, K):
    g = torch.Generator().manual_seed(M)
    X = torch.randn(M, K, generator=g, dtype=torch.float64)
    lin = torch.nn.Linear(K, N).double()
    dY = torch.randn(M, N, generator=g, dtype=torch.float64)
    lin(X).backward(dY)
    dW, db = RC.gemm_wgrad(dY, X, alpha=1.0)
    assert float((dW - lin.weight.grad).abs().max()) <= 1e-12 * max(1.0, float(dW.abs().max()))
    assert float((db - lin.bias.grad).abs().max()) <= 1e-12 * max(1.0, float(db.abs().max()))
    dW2, db2 = RC.gemm_wgrad(dY, X, alpha=0.25)
    assert torch.equal(dW2, 0.25 * (dY.t() @ X)) and torch.equal(db2, 0.25 * dY.sum(0))
