"""CPU checks of the fp32 precision mode's public surface: the names CLIP.set_precision and
create_model accept, the CLIPEMBED_PRECISION environment default, and the C header's declarations."""
import os
import re

import pytest

import clipembed
from clipembed import model as M
from clipembed.pacl import open_clip_pacl, sparc

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "clipembed.h")


def test_set_precision_rejects_other_names():
    m = clipembed.CLIP(clipembed.get_model_config("ViT-L-14-336"))
    for bad in ("fp16", "amp", "FP32", "", None):
        with pytest.raises(ValueError, match="precision"):
            m.set_precision(bad)
    assert m.precision == "bf16"
    assert m.set_precision("fp32") is m and m.precision == "fp32"      # before .to(device): remembered
    assert m.set_precision("bf16").precision == "bf16"


@pytest.mark.parametrize("bad", ["fp16", "pure_fp16", "pure_bf16", "amp_bfloat16", "int8"])
def test_create_model_rejects_unsupported_precision(bad, monkeypatch):
    monkeypatch.delenv(M.PRECISION_ENV, raising=False)
    with pytest.raises(ValueError, match="fp32.*bf16"):
        clipembed.create_model("ViT-L-14-336", precision=bad)
    with pytest.raises(ValueError, match="fp32.*bf16"):
        clipembed.create_model_and_transforms("ViT-L-14-336", precision=bad)


def test_default_is_bf16_without_the_variable(monkeypatch):
    monkeypatch.delenv(M.PRECISION_ENV, raising=False)
    assert clipembed.create_model("ViT-L-14-336", precision=None).precision == "bf16"
    assert clipembed.create_model_and_transforms("ViT-L-14-336")[0].precision == "bf16"
    assert open_clip_pacl().clip_model.precision == "bf16"
    for name in ("bf16", "amp", "amp_bf16"):
        assert clipembed.create_model("ViT-L-14-336", precision=name).precision == "bf16"
    assert clipembed.create_model("ViT-L-14-336", precision="fp32").precision == "fp32"
    assert sparc(precision="fp32").clip_model.precision == "fp32"


def test_environment_selects_fp32(monkeypatch):
    monkeypatch.setenv(M.PRECISION_ENV, "fp32")
    assert clipembed.create_model("ViT-L-14-336").precision == "fp32"
    assert clipembed.create_model_and_transforms("ViT-L-14-336")[0].precision == "fp32"
    assert open_clip_pacl().clip_model.precision == "fp32"
    # an explicit argument wins over the variable
    assert clipembed.create_model("ViT-L-14-336", precision="bf16").precision == "bf16"
    monkeypatch.setenv(M.PRECISION_ENV, "fp16")
    with pytest.raises(ValueError, match=M.PRECISION_ENV):
        clipembed.create_model("ViT-L-14-336")


def test_header_declares_the_mode():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("ce_set_precision", "ce_kernel_gemm_f32", "ce_kernel_attention_f32"):
        assert re.search(r"^int\s+%s\s*\(" % name, src, re.M), name
    assert re.search(r"enum\s+ce_precision\s*\{\s*CE_PREC_BF16\s*=\s*0\s*,\s*CE_PREC_F32\s*=\s*1\s*\}", src)
    from clipembed import _lib
    assert (_lib.CE_PREC_BF16, _lib.CE_PREC_F32) == (0, 1)
    assert {"ce_set_precision", "ce_kernel_gemm_f32", "ce_kernel_attention_f32"} <= set(_lib.exported_symbols())
