"""The eval drivers' decisions in the fp32 precision mode, held to a FIXED bar per decision kind.

Same items, seeds, fixtures and scoring as tests/test_gpu_eval_dropin.py (eval_clip.py:49-65,296-331;
eval_pacl.py:49-57; eval_sparc.py:26-56), with the model built with precision="fp32" (the SPARC
models through CLIPEMBED_PRECISION=fp32 and no precision argument, as the reference's scripts
would).  For every kind and EVERY item |engine margin - reference margin| <= TOL[kind], and the
decision is identical for every item whose |reference margin| > TOL[kind].  No band derived from
the engine's own error.

TOL[kind] = 20 x the largest |margin(CPU oracle) - margin(fixture)| of that kind over the 40 items,
over the oracle's float32 runs at 8 and 16 threads and its float64 run (tools/exact_margin_noise.py;
figures in DESIGN.md, fp32 mode): what two correct implementations differ by, times 20 because the
MFMA sums K in one chain where the CPU sums in blocks (3-4x worse at K = 4096) and erff / expf
differ by an ulp or two.  For the eight kinds other than sparc_global / sparc_local TOL is below
the smallest reference margin, so all 40 decisions are asserted; those two have one item each with
a margin of 0.001 (the next: 0.019 / 0.030), and at most that one item may lie inside TOL."""
import os
import importlib.util

import numpy as np
import pytest
import torch

import clipembed
from clipembed import weights as W
from clipembed.model import PRECISION_ENV

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("mgp", os.path.join(HERE, "golden", "make_golden_preprocess.py"))
mgp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mgp)

# measured max |margin(oracle) - margin(fixture)| over the 40 items, logit units (python
# tools/exact_margin_noise.py):            f32 x 8 thr  f32 x 16 thr  float64     -> 20 x the largest
TOL = {
    "whatsup": 20 * 1.485e-5,            # 1.392e-5    1.485e-5      1.002e-5    (smallest reference margin 2.7e-2)
    "mmvp": 20 * 7.140e-6,               # 7.140e-6    6.219e-6      5.503e-6    (2.6e-3)
    "mmvp2": 20 * 8.640e-6,              # 5.975e-6    6.620e-6      8.640e-6    (1.2e-1)
    "pacl": 20 * 1.137e-5,               # 2.384e-6    4.888e-6      1.137e-5    (5.6e-2)
    "pacl_rope": 20 * 1.018e-5,          # 1.431e-6    5.722e-6      1.018e-5    (4.8e-2)
    "pacl_rope_after": 20 * 1.032e-5,    # 2.444e-6    4.709e-6      1.032e-5    (2.0e-1)
    "sparc_global": 20 * 3.927e-6,       # 1.863e-6    1.863e-6      3.927e-6    (9.9e-4, then 1.9e-2)
    "sparc_local": 20 * 3.994e-6,        # 1.863e-6    1.863e-6      3.994e-6    (1.1e-3, then 3.0e-2)
    "sparc_rope_global": 20 * 3.013e-6,  # 1.118e-6    1.118e-6      3.013e-6    (1.4e-1)
    "sparc_rope_local": 20 * 3.721e-6,   # 2.235e-6    2.235e-6      3.721e-6    (9.9e-2)
}
# (no alignment weight crossed sigma between the three CPU runs: the live weight nearest to sigma sits
# 2.8e-6 above it, and the SPARC margins agree as closely as the others.  The measured TOL of
# sparc_global / sparc_local is also below their smallest margins, so in practice no item is inside)
MAY_EXCLUDE = {"sparc_global": 1, "sparc_local": 1}      # items allowed inside TOL (every other kind: 0)


def _items():
    # the item table of the generator (parsed without importing it: its imports need the reference)
    src = open(os.path.join(HERE, "golden", "make_golden_eval.py")).read()
    start = src.index("ITEMS = [")
    ns = {}
    exec(src[start:src.index("]\n", start) + 1], ns)
    return ns["ITEMS"]


ITEMS = _items()
DEVICE = "cuda:0"


def pil(k):
    from PIL import Image
    i, h, w = ITEMS[k][:3]
    return Image.fromarray(mgp.image(i, h, w))


def _check(kind, got_margin, ref_margin, got_dec, ref_dec):
    got_margin, ref_margin = np.asarray(got_margin, np.float64), np.asarray(ref_margin, np.float64)
    got_dec, ref_dec = np.asarray(got_dec), np.asarray(ref_dec)
    tol = TOL[kind]
    d = np.abs(got_margin - ref_margin)
    inside = np.abs(ref_margin) <= tol
    print(f"{kind}: max |engine margin - reference margin| {d.max():.3e} (item {int(d.argmax())}), TOL {tol:.3e}, "
          f"smallest |reference margin| {np.abs(ref_margin).min():.3e}, items inside TOL {int(inside.sum())}, "
          f"decisions identical {int((got_dec == ref_dec).sum())}/{got_dec.size}")
    assert got_dec.size == 40
    assert int(inside.sum()) <= MAY_EXCLUDE.get(kind, 0), f"{kind}: {int(inside.sum())} reference margins inside TOL"
    assert (d <= tol).all(), f"{kind}: margins differ by up to {d.max():.3e} > {tol:.3e} (items {np.nonzero(d > tol)[0].tolist()})"
    assert np.array_equal(got_dec[~inside], ref_dec[~inside]), \
        f"{kind}: decisions differ at items {np.nonzero((got_dec != ref_dec) & ~inside)[0].tolist()}"


@pytest.fixture(scope="module")
def clip_sd():
    return W.synthetic_state_dict(clipembed.get_model_config("ViT-L-14-336"))


@pytest.fixture(scope="module")
def heads_sd():
    return W.synthetic_pacl_heads(clipembed.get_model_config("ViT-L-14-336").with_pacl(768))


@pytest.fixture(scope="module")
def drop_in(clip_sd):
    """`model, image_processor, _ = oc.create_model_and_transforms(..., precision="fp32")`, oc = clipembed."""
    model, image_processor, _ = clipembed.create_model_and_transforms("ViT-L-14-336", precision="fp32")
    model.load_state_dict(clip_sd)
    model.to(torch.device(DEVICE))
    model.eval()
    assert model.precision == "fp32"
    return model, image_processor


def _mmvp(model, process, image_processor, ids, images, boxes):
    margins, preds = [], []
    for j in range(len(ITEMS) // 2):
        texts = torch.from_numpy(ids[j]).to(DEVICE)
        pix = []
        for q, im in enumerate(images(j)):
            pix.append(process.preprocess_image(im).unsqueeze(0).to(DEVICE))
            assert np.array_equal(image_processor.last_boxes[0], boxes[2 * j + q])
        imgs = torch.cat(pix, dim=0)
        with torch.no_grad():
            image_features = model.encode_image(imgs)
            text_features = model.encode_text(texts)
            image_features /= image_features.norm(dim=-1, keepdim=True)
            text_features /= text_features.norm(dim=-1, keepdim=True)
            text_probs = (100.0 * text_features @ image_features.T).softmax(dim=-1)
        probs1, probs2 = text_probs[0].cpu().numpy(), text_probs[1].cpu().numpy()
        preds.append([int(probs1[0] > 0.5), int(probs2[0] > 0.5)])
        margins.append([float(np.log(probs1[0] / probs1[1])), float(np.log(probs2[0] / probs2[1]))])
    return np.ravel(margins), np.ravel(preds)


def test_whatsup(drop_in, golden):
    g = golden("eval_decisions")
    model, image_processor = drop_in
    process = clipembed.prepare_data_clip(image_processor)          # eval_clip.py:24
    torch.manual_seed(1234)
    margins, correct = [], []
    for k in range(len(ITEMS)):                                     # eval_clip.py:49-65
        input_pixels = process.preprocess_image(pil(k)).unsqueeze(0).to(DEVICE)
        assert np.array_equal(image_processor.last_boxes[0], g["whatsup_boxes"][k])
        tokenized_text = torch.from_numpy(g["ids"][k]).to(DEVICE)
        with torch.no_grad():
            image_features = model.encode_image(input_pixels)
            text_features = model.encode_text(tokenized_text)
            image_features /= image_features.norm(dim=-1, keepdim=True)
            text_features /= text_features.norm(dim=-1, keepdim=True)
            text_probs = (100.0 * image_features @ text_features.T).softmax(dim=-1)
        correct.append(1 if text_probs[0][0] > text_probs[0][1] else 0)
        margins.append(float(torch.log(text_probs[0][0] / text_probs[0][1])))
    p = g["whatsup_probs"].astype(np.float64)
    _check("whatsup", margins, np.log(p[:, 0] / p[:, 1]), correct, g["whatsup_correct"])


def test_mmvp(drop_in, golden):
    g = golden("eval_decisions")
    model, image_processor = drop_in
    process = clipembed.prepare_data_clip(image_processor)
    torch.manual_seed(4321)                                         # eval_clip.py:296-331
    margins, preds = _mmvp(model, process, image_processor, g["mmvp_ids"], lambda j: (pil(2 * j), pil(2 * j + 1)),
                           g["mmvp_boxes"])
    m = g["mmvp_probs"].astype(np.float64)
    _check("mmvp", margins, np.ravel(np.log(m[:, :, 0] / m[:, :, 1])), preds, np.ravel(g["mmvp_pred_img1"]))


def test_mmvp2(drop_in, golden):
    from PIL import Image
    g = golden("eval_decisions")
    model, image_processor = drop_in
    process = clipembed.prepare_data_clip(image_processor)

    def images(j):      # a gradient image against a single-colour one (make_golden_eval.py mmvp2)
        (i0, h0, w0), (i1, h1, w1) = ITEMS[2 * j][:3], ITEMS[2 * j + 1][:3]
        a, b = (mgp.image(i0, h0, w0), mgp.solid_image(i1, h1, w1)) if j % 2 == 0 else \
               (mgp.solid_image(i0, h0, w0), mgp.image(i1, h1, w1))
        return Image.fromarray(a), Image.fromarray(b)

    torch.manual_seed(4322)
    margins, preds = _mmvp(model, process, image_processor, g["mmvp2_ids"], images, g["mmvp2_boxes"])
    m = g["mmvp2_probs"].astype(np.float64)
    _check("mmvp2", margins, np.ravel(np.log(m[:, :, 0] / m[:, :, 1])), preds, np.ravel(g["mmvp2_pred_img1"]))


@pytest.fixture(scope="module")
def pacl_model(clip_sd, heads_sd):
    from clipembed.pacl import open_clip_pacl
    model = open_clip_pacl("ViT-L-14-336", clip_state_dict=clip_sd, precision="fp32")
    model.load_state_dict(heads_sd)
    model.to(torch.device(DEVICE))
    return model


@pytest.mark.parametrize("kind", ["pacl", "pacl_rope", "pacl_rope_after"])
def test_pacl(pacl_model, golden, kind):
    """eval_pacl.py:49-57 with open_clip_pacl and the RoPE variants its model path selects
    (eval_pacl.py:372-377): one engine, the variant's class attributes (weighting, RoPE position)."""
    from clipembed import pacl as PM
    cls = {"pacl": PM.open_clip_pacl, "pacl_rope": PM.open_clip_pacl_rope, "pacl_rope_after": PM.open_clip_pacl_rope_after}[kind]
    g = golden("eval_decisions") if kind == "pacl" else golden("eval_pacl_variants")
    model = pacl_model
    model.weight_mode, model.rope = cls.weight_mode, cls.rope
    process = clipembed.prepare_data(base_model="ViT-L-14-336")     # eval_pacl.py:19
    margins, correct = [], []
    try:
        for k in range(len(ITEMS)):
            input_pixels = process.preprocess_image(pil(k)).unsqueeze(0).to(DEVICE)
            tokenized_text = torch.from_numpy(g["ids"][k]).to(DEVICE)
            with torch.no_grad():
                image_features, text_features = model(input_pixels, tokenized_text)
                text_probs = 100.0 * image_features @ text_features.T
            correct.append(1 if text_probs[0][0] > text_probs[1][1] else 0)
            margins.append(float(text_probs[0][0] - text_probs[1][1]))
    finally:
        model.weight_mode, model.rope = PM.open_clip_pacl.weight_mode, PM.open_clip_pacl.rope
    s = g[f"{kind}_scores"].astype(np.float64)
    _check(kind, margins, s[:, 0, 0] - s[:, 1, 1], correct, g[f"{kind}_correct"])


@pytest.fixture(scope="module")
def sparc_model(clip_sd, heads_sd):
    """Built with NO precision argument under CLIPEMBED_PRECISION=fp32, as the reference's scripts
    (create_model_and_transforms("ViT-L-14-336", pretrained='openai'), pacl.py:399) would be."""
    from clipembed.pacl import sparc
    old = os.environ.get(PRECISION_ENV)
    os.environ[PRECISION_ENV] = "fp32"
    try:
        model = sparc(sigma=1.0 / 576, cfg=clipembed.get_model_config("ViT-L-14-336"), clip_state_dict=clip_sd)
    finally:
        if old is None:
            del os.environ[PRECISION_ENV]
        else:
            os.environ[PRECISION_ENV] = old
    assert model.clip_model.precision == "fp32"
    model.load_state_dict(heads_sd)
    model.to(torch.device(DEVICE))
    return model


@pytest.mark.parametrize("tag", ["sparc", "sparc_rope"])
@pytest.mark.parametrize("local", [False, True])
def test_sparc(sparc_model, golden, tag, local):
    """eval_sparc.py:26-56: model.scoring(1 image, 2 captions, local), correct = s[0][0] > s[1][1];
    margins in 100 x cosine units.  sparc_rope = sparc with RoPE before the visual head (pacl.py:480-484)."""
    from clipembed import pacl as PM
    g = golden("eval_sparc_decisions")
    model = sparc_model
    model.rope = (PM.sparc_rope if tag == "sparc_rope" else PM.sparc).rope
    process = clipembed.prepare_data(base_model="ViT-L-14-336")
    margins, correct = [], []
    try:
        for k in range(len(ITEMS)):
            input_pixels = process.preprocess_image(pil(k)).unsqueeze(0).to(DEVICE)
            tokenized_text = torch.from_numpy(g["ids"][k]).to(DEVICE)
            with torch.no_grad():
                s = model.scoring(input_pixels, tokenized_text, local=local)
            correct.append(1 if s[0][0] > s[1][1] else 0)
            margins.append(100.0 * float(s[0][0] - s[1][1]))
    finally:
        model.rope = PM.sparc.rope
    key = f"{tag}_{'local' if local else 'global'}"
    ref = g[f"{key}_scores"].astype(np.float64)
    _check(key, margins, 100.0 * (ref[:, 0, 0] - ref[:, 1, 1]), correct, g[f"{key}_correct"])
