"""The fp32 precision mode end to end (CLIP.set_precision("fp32"), ce_set_precision): full-depth
ViT-L/14-336 against the reference's f32 run (tests/golden/clip_full.npz), switching between the
modes, and the error when the mode's f32 weight copies are missing.

Metric: relative L2 error per row, ||got - ref|| / ||ref|| in float64 (cosine distance is quadratic
in the error and says nothing at this level)."""
import ctypes

import numpy as np
import pytest
import torch

import clipembed
from clipembed import _lib, weights as W
from clipembed.config import get_model_config
from clipembed.model import _ptr, _stream

pytestmark = pytest.mark.gpu

ROWS_V = [0, 1, 23, 24, 287, 300, 551, 575]
ROWS_T = [0, 1, 5, 20, 40, 76]

# Two correct f32 implementations against the fixture, the same metric, measured on the CPU with
# tools/exact_margin_noise.py --parity (oracle/clip_torch_cpu.py at full depth):
#                     image_pooled  text_pooled  image_tokens_rows  text_tokens_rows
#   f32,  8 threads     5.03e-7       1.10e-6        3.95e-7            1.16e-6
#   f32, 16 threads     5.35e-7       1.09e-6        3.95e-7            1.16e-6
#   float64             4.74e-7       9.26e-7        6.12e-7            1.01e-6
# The bar is 20 x the largest (1.161e-6): the MFMA sums K in one chain where the CPU sums in blocks
# (3-4x worse at K = 4096), and erff / expf differ from the CPU's by an ulp or two.
REL_L2_BAR = 20 * 1.161e-6


def rel_l2(a, b):
    a = np.asarray(a, np.float64).reshape(-1, a.shape[-1])
    b = np.asarray(b, np.float64).reshape(-1, b.shape[-1])
    return float((np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)).max())


def make_model(cfg, precision=None):
    m = clipembed.CLIP(cfg)
    if precision:
        m.set_precision(precision)
    m.load_state_dict(W.synthetic_state_dict(cfg))
    return m.to("cuda")


def test_full_depth_fp32_vs_golden(golden):
    g = golden("clip_full")
    m = make_model(get_model_config("ViT-L-14-336"), "fp32")
    imgs = torch.from_numpy(W.synthetic_images(2, seed=1000))
    caps = torch.from_numpy(g["captions"])
    m.visual.output_tokens = True
    m.output_text_tokens = True
    pi, ti = m.encode_image(imgs)
    pt, tt = m.encode_text(caps)
    pi, ti, pt, tt = (x.cpu().numpy() for x in (pi, ti, pt, tt))
    errs = {"image_pooled": rel_l2(pi, g["image_pooled"]), "text_pooled": rel_l2(pt, g["text_pooled"]),
            "image_tokens_rows": rel_l2(ti[:, ROWS_V], g["image_tokens_rows"]),
            "text_tokens_rows": rel_l2(tt[:, ROWS_T], g["text_tokens_rows"])}
    print("fp32 mode, relative L2 per row vs clip_full:", {k: f"{v:.3e}" for k, v in errs.items()},
          f"bar {REL_L2_BAR:.3e}")
    for k, v in errs.items():
        assert v <= REL_L2_BAR, f"{k}: {v:.3e} > {REL_L2_BAR:.3e}"
    # pooled-only calls take the same path (no pooled prune in this mode): identical rows
    m.visual.output_tokens = False
    m.output_text_tokens = False
    assert np.array_equal(m.encode_image(imgs).cpu().numpy(), pi)
    assert np.array_equal(m.encode_text(caps).cpu().numpy(), pt)


def _outputs(m, imgs, caps):
    m.visual.output_tokens = True
    m.output_text_tokens = True
    try:
        pi, ti = m.encode_image(imgs)
        pt, tt = m.encode_text(caps)
    finally:
        m.visual.output_tokens = False
        m.output_text_tokens = False
    return [x.cpu().numpy() for x in (pi, ti, pt, tt, m.encode_image(imgs), m.encode_text(caps))]


def test_switching_modes():
    """bf16 -> fp32 -> bf16 on a live engine: the bf16 outputs come back bitwise, the fp32 ones differ
    from them (a mode that silently did nothing would not) and sit nearer the f32 oracle; the timing
    tags tell the two paths apart."""
    from oracle import clip_oracle as O
    cfg = get_model_config("ViT-L-14-336").with_depth(1, 1)
    m = make_model(cfg)
    imgs = torch.from_numpy(W.synthetic_images(2, seed=1000))
    caps = torch.from_numpy(W.synthetic_captions(3, seed=2000))
    before = _outputs(m, imgs, caps)
    m.set_precision("fp32")
    m.engine.set_timing(True)
    try:
        exact = _outputs(m, imgs, caps)
        torch.cuda.synchronize()
        names = {k["name"] for k in m.engine.kernel_stats()}
    finally:
        m.engine.set_timing(False)
    assert {"gemm_patch_f32", "gemm_qkv_v_f32", "attn_v_f32", "gemm_out_v_f32", "gemm_fc_v_f32", "gemm_proj_v_f32",
            "gemm_qkv_t_f32", "attn_t_f32", "gemm_fc_t_f32"} <= names, names
    assert not {"gemm_qkv_v", "attn_v", "gemm_qkv_t", "attn_t", "gemm_patch"} & names, names
    m.set_precision("bf16")
    after = _outputs(m, imgs, caps)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    for a, x in zip(before, exact):
        assert not np.array_equal(a, x)
    sd = W.synthetic_state_dict(cfg)
    ri, rt = O.encode_image(sd, imgs.numpy(), cfg), O.encode_text(sd, caps.numpy(), cfg)
    print(f"one block, relative L2 vs the f32 oracle: image fp32 {rel_l2(exact[0], ri):.3e} / bf16 {rel_l2(before[0], ri):.3e}, "
          f"text fp32 {rel_l2(exact[2], rt):.3e} / bf16 {rel_l2(before[2], rt):.3e}")
    # (bf16 rounds operands to 2^-9 relative, f32 to 2^-24: the fp32 rows must be far nearer)
    assert rel_l2(exact[0], ri) < 0.05 * rel_l2(before[0], ri)
    assert rel_l2(exact[2], rt) < 0.05 * rel_l2(before[2], rt)
    # Engine.set_precision reports the previous mode
    assert m.engine.set_precision("bf16") == "bf16"


def test_missing_f32_copies_is_an_error():
    """Weights loaded in bf16 mode, then CE_PREC_F32 set through the C ABI with no reload: the encode
    call names a tensor and returns CE_ERR_STATE; it does not fall back to the bf16 weights."""
    cfg = get_model_config("ViT-L-14-336").with_depth(1, 1)
    m = make_model(cfg)
    e = m.engine
    L = _lib.lib()
    prev = ctypes.c_int(-1)
    assert L.ce_set_precision(e.h, _lib.CE_PREC_F32, ctypes.byref(prev)) == _lib.CE_OK
    assert prev.value == _lib.CE_PREC_BF16
    ids = torch.from_numpy(W.synthetic_captions(2, seed=5)).cuda()
    out = torch.full((2, cfg.embed_dim), 7.0, device="cuda")
    rc = L.ce_encode_text(e.h, _stream(e.device), _ptr(ids), 2, cfg.text.context_length, 0, _ptr(out), None, 0)
    msg = L.ce_last_error().decode()
    assert rc == _lib.CE_ERR_STATE, (rc, msg)
    assert "transformer.resblocks.0." in msg and "f32" in msg, msg
    pix = torch.from_numpy(W.synthetic_images(1, seed=6)).cuda()
    rc = L.ce_encode_image(e.h, _stream(e.device), _ptr(pix), _lib.CE_F32, 1, 0, _ptr(out), None, 0)
    assert rc == _lib.CE_ERR_STATE and "visual." in L.ce_last_error().decode()
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    assert L.ce_set_precision(e.h, 5, None) == _lib.CE_ERR_INVALID
    # loading again in the mode makes it run
    m.set_precision("fp32")
    assert torch.isfinite(m.encode_text(ids)).all()
