"""The fp32 mode's kernels (csrc/exact.hip) through their C-ABI entry points, against float64 torch
on the CPU.

GEMM bar, per element: |got - ref64| <= 1e-6 * (sum_k |a_k w_k| + |bias| + |resid|).  The f32-input
MFMA is a k-ordered fmaf chain; such a chain measures 3.5e-7 * sum|a b| against float64 at K = 4096
(0.75 - 1.5e-7 at K <= 1024), and the bar is that with 3x margin.  With an activation the bar also
takes 4x the error torch's own f32 F.gelu / sigmoid make against float64 on the same pre-activations.

Attention bar: max abs error against float64 <= 4x the max abs error of torch's f32 CPU attention
against float64 on the same inputs.  The lengths cross every edge of the kernel's 32-query / 32-key
tiles and include the two real ones (77 causal, 577)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from clipembed import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda"


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def act64(pre, act):
    if act == 1:
        return F.gelu(pre)
    if act == 2:
        return pre * torch.sigmoid(1.702 * pre)
    return pre


@pytest.mark.parametrize("M,N,K,pad", [(1, 64, 32, 0), (33, 64, 64, 0), (130, 192, 640, 8), (577, 64, 1024, 0)])
@pytest.mark.parametrize("variant", ["plain", "bias_gelu", "bias_qgelu", "bias_resid_alias"])
def test_gemm_f32(M, N, K, pad, variant):
    g = torch.Generator(device="cpu").manual_seed(M * 7 + N * 3 + K)
    lda = K + pad
    Abuf = torch.randn(M, lda, generator=g)
    A = Abuf[:, :K]
    W = torch.randn(N, K, generator=g) * K ** -0.5
    bias = torch.randn(N, generator=g) * 0.1 if variant != "plain" else None
    resid = torch.randn(M, N, generator=g) if variant == "bias_resid_alias" else None
    act = {"bias_gelu": 1, "bias_qgelu": 2}.get(variant, 0)
    dA, dW = Abuf.to(DEV), W.to(DEV)
    dbias = bias.to(DEV) if bias is not None else None
    if resid is not None:
        out = resid.to(DEV).clone()          # the residual aliases the output
        dres = out
    else:
        out = torch.full((M, N), float("nan"), device=DEV)
        dres = None
    _lib.call("ce_kernel_gemm_f32", S(), P(dA), lda, P(dW), M, N, K, P(dbias), act, P(dres), P(out), N)
    torch.cuda.synchronize()
    got = out.cpu().double()
    pre = A.double() @ W.double().t()
    mag = A.double().abs() @ W.double().abs().t()
    if bias is not None:
        pre = pre + bias.double()
        mag = mag + bias.double().abs()
    ref = act64(pre, act)
    tol = 1e-6 * mag
    if act:
        pre32 = pre.float()
        act_err = (act64(pre32, act).double() - act64(pre32.double(), act)).abs().max().item()
        tol = tol + 4 * act_err
    if resid is not None:
        ref = ref + resid.double()
        tol = tol + 1e-6 * resid.double().abs()
    err = (got - ref).abs()
    worst = (err / tol.clamp_min(1e-300)).max().item()
    print(f"gemm_f32 {M}x{N}x{K} {variant}: max err {err.max().item():.3e}, worst err/tol {worst:.3f}")
    assert torch.isfinite(got).all()
    assert (err <= tol).all(), f"max err {err.max().item():.3e}, worst err/tol {worst:.3f}"


@pytest.mark.parametrize("B,H,L,causal", [(2, 2, 1, False), (2, 2, 17, True), (2, 2, 33, False), (1, 2, 65, False),
                                          (2, 2, 77, True), (1, 1, 577, False)])
def test_attention_f32(B, H, L, causal):
    g = torch.Generator(device="cpu").manual_seed(B * 1000 + H * 100 + L)
    qkv = torch.randn(B * L, 3 * H * 64, generator=g)
    out = torch.full((B * L, H * 64), float("nan"), device=DEV)
    _lib.call("ce_kernel_attention_f32", S(), P(qkv.to(DEV)), P(out), B, L, H, 1 if causal else 0)
    torch.cuda.synchronize()
    got = out.cpu().double()
    q, k, v = (t.reshape(B, L, H, 64).transpose(1, 2) for t in qkv.split(H * 64, dim=1))    # [B, H, L, 64]
    s = q.double() @ k.double().transpose(-1, -2) / 8.0
    if causal:
        s = s.masked_fill(torch.ones(L, L, dtype=torch.bool).triu(1), float("-inf"))
    ref = (torch.softmax(s, dim=-1) @ v.double()).transpose(1, 2).reshape(B * L, H * 64)
    t32 = F.scaled_dot_product_attention(q, k, v, is_causal=causal).transpose(1, 2).reshape(B * L, H * 64)
    bar = 4 * (t32.double() - ref).abs().max().item()
    err = (got - ref).abs().max().item()
    print(f"attention_f32 B{B} H{H} L{L} causal={causal}: max err {err:.3e}, bar {bar:.3e}")
    assert torch.isfinite(got).all()
    assert err <= bar, f"max err {err:.3e} vs bar {bar:.3e}"
    if causal:
        # row 0 sees key 0 only
        got0 = got.reshape(B, L, H * 64)[:, 0]
        v0 = v.transpose(1, 2).reshape(B, L, H * 64)[:, 0].double()
        assert ((got0 - v0).abs() <= 1e-6 * v0.abs()).all()
