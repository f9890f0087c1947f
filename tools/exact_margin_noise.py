"""How far two correct implementations of the eval flows differ: the CPU measurement behind the bars
of the fp32 mode's tests (tests/test_gpu_exact_eval.py, tests/test_gpu_exact_parity.py).

Runs the CPU oracle (oracle/clip_torch_cpu.py: the reference's ATen calls) at full depth on the 40
items of tests/golden/make_golden_eval.py in float32 at several thread counts and in float64, scores
the ten decision kinds as the eval drivers do, and prints per kind the largest |margin(oracle) -
margin(fixture)| over the items (fixtures: tests/golden/eval_decisions.npz, eval_sparc_decisions.npz,
eval_pacl_variants.npz, the reference's own f32 run).  `--parity` prints instead the relative L2
error per row of the oracle's pooled / token rows against tests/golden/clip_full.npz.  A test bar is
20 x the largest value over the runs (DESIGN.md, fp32 mode).

The PACL / SPARC heads (oracle/clip_oracle.py restates them in NumPy float32 only) are restated here
in torch so that the float64 run covers them; the RoPE tables keep the reference's f32 arithmetic.
CPU only; reads the repository and its fixtures.

    python tools/exact_margin_noise.py --runs f32:8 f32:16 f64:8 [--items 40] [--kinds whatsup mmvp ...]
    python tools/exact_margin_noise.py --parity --runs f32:8 f32:16 f64:8
"""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "clip-embeds_amd"), REPO]
GOLDEN = os.path.join(REPO, "tests", "golden")

from clipembed import weights as W  # noqa: E402
from clipembed.config import get_model_config  # noqa: E402
from oracle import preprocess_oracle as P  # noqa: E402
from oracle.clip_torch_cpu import TorchCLIP  # noqa: E402

KINDS = ["whatsup", "mmvp", "mmvp2", "pacl", "pacl_rope", "pacl_rope_after", "sparc_global", "sparc_local",
         "sparc_rope_global", "sparc_rope_local"]
ROWS_V = [0, 1, 23, 24, 287, 300, 551, 575]
ROWS_T = [0, 1, 5, 20, 40, 76]
SIGMA = 1.0 / 576


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MGP = _load("make_golden_preprocess")


def items():
    src = open(os.path.join(GOLDEN, "make_golden_eval.py")).read()
    start = src.index("ITEMS = [")
    ns = {}
    exec(src[start:src.index("]\n", start) + 1], ns)
    return ns["ITEMS"]


class Oracle(TorchCLIP):
    """oracle/clip_torch_cpu.py with a dtype and the token rows (its blocks, unchanged)."""

    def __init__(self, sd, cfg, dtype):
        super().__init__(sd, cfg)
        self.dtype = dtype
        self.w = {k: v.to(dtype) for k, v in self.w.items()}

    @torch.inference_mode()
    def image(self, pixels):
        """(pooled [B, E], tokens [B, P, D]) of CLIP.encode_image with visual.output_tokens."""
        v, w = self.cfg.vision, self.w
        x = torch.as_tensor(pixels).to(self.dtype)
        x = F.conv2d(x, w["visual.conv1.weight"], stride=v.patch_size)
        x = x.reshape(x.shape[0], x.shape[1], -1).permute(0, 2, 1)
        x = torch.cat([w["visual.class_embedding"].expand(x.shape[0], 1, -1), x], 1) + w["visual.positional_embedding"]
        x = F.layer_norm(x, (v.width,), w["visual.ln_pre.weight"], w["visual.ln_pre.bias"], 1e-5)
        for i in range(v.layers):
            x = self._block(x, f"visual.transformer.resblocks.{i}.", v.heads, None)
        x = F.layer_norm(x, (v.width,), w["visual.ln_post.weight"], w["visual.ln_post.bias"], 1e-5)
        return x[:, 0] @ w["visual.proj"], x[:, 1:]

    @torch.inference_mode()
    def text(self, ids):
        """(pooled [B, E], tokens [B, T, D]) of CLIP.encode_text with output_text_tokens."""
        t, w = self.cfg.text, self.w
        ids = torch.as_tensor(ids).long()
        L = ids.shape[1]
        x = w["token_embedding.weight"][ids] + w["positional_embedding"]
        mask = torch.full((L, L), float("-inf"), dtype=self.dtype).triu_(1)
        for i in range(t.layers):
            x = self._block(x, f"transformer.resblocks.{i}.", t.heads, mask)
        x = F.layer_norm(x, (t.width,), w["ln_final.weight"], w["ln_final.bias"], 1e-5)
        return x[torch.arange(x.shape[0]), ids.argmax(dim=-1)] @ w["text_projection"], x


# ---- heads (pacl.py:20-50,70-79,120-209,453-478; as oracle/clip_oracle.py, any dtype) -------------
def rope(x):
    B, L, D = x.shape
    e = (np.arange(0, D, 2, dtype=np.float32) / np.float32(D)).astype(np.float32)
    inv = (np.float32(1.0) / (10000.0 ** e.astype(np.float64)).astype(np.float32)).astype(np.float32)
    ang = (np.arange(L, dtype=np.float32)[:, None] * inv[None, :]).astype(np.float32)
    s = torch.from_numpy(np.sin(ang).astype(np.float32)).to(x.dtype)
    c = torch.from_numpy(np.cos(ang).astype(np.float32)).to(x.dtype)
    x1, x2 = x[..., 0::2], x[..., 1::2]
    return torch.cat([x1 * c - x2 * s, x1 * s + x2 * c], dim=-1)


def visual_head(h, tokens):
    x = F.layer_norm(tokens, (tokens.shape[-1],), h["visual_projection.0.weight"], h["visual_projection.0.bias"], 1e-5)
    lin = F.linear(x, h["visual_projection.2.linear_projection.0.weight"], h["visual_projection.2.linear_projection.0.bias"])
    nl = F.gelu(F.linear(x, h["visual_projection.2.non_linear_projection.0.weight"],
                         h["visual_projection.2.non_linear_projection.0.bias"]))
    return lin + F.linear(nl, h["visual_projection.2.non_linear_projection.2.weight"],
                          h["visual_projection.2.non_linear_projection.2.bias"])


def text_head(h, t):
    x = F.layer_norm(t, (t.shape[-1],), h["text_projection.0.weight"], h["text_projection.0.bias"], 1e-5)
    return F.linear(x, h["text_projection.2.weight"], h["text_projection.2.bias"])


def pacl_scores(vp, tp, sigmoid, rope_after):
    """100 I T^T of open_clip_pacl.forward for 1 image x 2 captions (pacl.py:120-145,199-209)."""
    tn = F.normalize(tp, dim=-1)
    src = rope(vp) if rope_after else vp
    rows = []
    for r in range(tp.shape[0]):
        if sigmoid:
            wgt = torch.sigmoid(10.0 * (F.normalize(src[0], dim=-1) @ tn[r]))
            rows.append((vp[0] * wgt[:, None]).sum(0))
        else:
            rows.append(vp[0].sum(0))
    img = F.normalize(torch.stack(rows), dim=-1)
    return 100.0 * img @ tn.T


def sparc_scores(v, l, local):
    """sparc.scoring (pacl.py:453-478 and the scoring head): v [2, P, D] (the image repeated), l [2, T, D]."""
    sim = torch.einsum("btd,bpd->btp", l, v)
    mn, mx = sim.min(-1, keepdim=True).values, sim.max(-1, keepdim=True).values
    s = (sim - mn) / (mx - mn + 1e-8)
    s = torch.where(s < SIGMA, torch.zeros_like(s), s)
    wgt = s / (s.sum(-1, keepdim=True) + 1e-8)
    g = F.normalize(torch.einsum("btp,bpd->btd", wgt, v), dim=-1)
    gt = F.normalize(F.normalize(l, dim=-1).mean(1), dim=-1)
    gi = F.normalize((g if local else v).mean(1), dim=-1)
    return gi @ gt.T, s


def clip_margins(fi, ft, t2i):
    fi, ft = F.normalize(fi.double(), dim=-1), F.normalize(ft.double(), dim=-1)
    z = 100.0 * (ft @ fi.T if t2i else fi @ ft.T)
    return (z[:, 0] - z[:, 1]).tolist() if t2i else [float(z[0, 0] - z[0, 1])]


def run_kinds(o, heads, kinds, n_items):
    IT = items()[:n_items]
    g = dict(np.load(os.path.join(GOLDEN, "eval_decisions.npz")))
    gs = dict(np.load(os.path.join(GOLDEN, "eval_sparc_decisions.npz")))
    gp = dict(np.load(os.path.join(GOLDEN, "eval_pacl_variants.npz")))
    out = {}
    img = lambda k: MGP.image(*IT[k][:3])
    if "whatsup" in kinds:
        m = []
        for k in range(len(IT)):
            fi, _ = o.image(P.clip_train_preprocess(img(k), g["whatsup_boxes"][k])[None])
            m += clip_margins(fi, o.text(g["ids"][k])[0], False)
        p = g["whatsup_probs"][:len(IT)].astype(np.float64)
        out["whatsup"] = (np.array(m), np.log(p[:, 0] / p[:, 1]))
    for kind in ("mmvp", "mmvp2"):
        if kind not in kinds:
            continue
        m = []
        for j in range(len(IT) // 2):
            if kind == "mmvp":
                ims = (img(2 * j), img(2 * j + 1))
            else:
                (i0, h0, w0), (i1, h1, w1) = IT[2 * j][:3], IT[2 * j + 1][:3]
                ims = (MGP.image(i0, h0, w0), MGP.solid_image(i1, h1, w1)) if j % 2 == 0 else \
                      (MGP.solid_image(i0, h0, w0), MGP.image(i1, h1, w1))
            pix = np.stack([P.clip_train_preprocess(im, g[f"{kind}_boxes"][2 * j + q]) for q, im in enumerate(ims)])
            m += clip_margins(o.image(pix)[0], o.text(g[f"{kind}_ids"][j])[0], True)
        p = g[f"{kind}_probs"][:len(IT) // 2].astype(np.float64)
        out[kind] = (np.array(m), np.ravel(np.log(p[:, :, 0] / p[:, :, 1])))
    head_kinds = [k for k in kinds if k.startswith(("pacl", "sparc"))]
    if head_kinds:
        m = {k: [] for k in head_kinds}
        cross = {}
        for k in range(len(IT)):
            _, tok = o.image(P.pacl_eval_preprocess(img(k))[None])
            tpool, ttok = o.text(g["ids"][k])
            vp, vpr = visual_head(heads, tok), visual_head(heads, rope(tok))
            tp = text_head(heads, tpool)
            lt = text_head(heads, ttok)
            for kind in head_kinds:
                if kind.startswith("pacl"):
                    z = pacl_scores(vpr if kind == "pacl_rope" else vp, tp, kind == "pacl_rope_after",
                                    kind == "pacl_rope_after")
                    m[kind].append(float(z[0, 0] - z[1, 1]))
                else:
                    v = (vpr if "rope" in kind else vp).expand(2, -1, -1)
                    z, s = sparc_scores(v, lt, kind.endswith("local"))
                    m[kind].append(100.0 * float(z[0, 0] - z[1, 1]))
                    # the thresholded weights nearest to sigma on either side (a crossing flips the weight to 0)
                    live = s[s > 0]
                    cross.setdefault(kind, []).append(float((live - SIGMA).min()) if live.numel() else float("nan"))
        for kind in head_kinds:
            if kind == "pacl":
                sc = g["pacl_scores"]
            elif kind.startswith("pacl"):
                sc = gp[f"{kind}_scores"]
            else:
                sc = gs[f"{kind}_scores"]
            sc = sc[:len(IT)].astype(np.float64)
            scale = 1.0 if kind.startswith("pacl") else 100.0
            out[kind] = (np.array(m[kind]), scale * (sc[:, 0, 0] - sc[:, 1, 1]))
        out["_sigma_gap"] = cross
    return out


def rel_l2(a, b):
    a = np.asarray(a, np.float64).reshape(-1, a.shape[-1])
    b = np.asarray(b, np.float64).reshape(-1, b.shape[-1])
    return float((np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)).max())


def run_parity(o):
    g = dict(np.load(os.path.join(GOLDEN, "clip_full.npz")))
    pi, ti = o.image(W.synthetic_images(2, seed=1000))
    pt, tt = o.text(g["captions"])
    return {"image_pooled": rel_l2(pi.numpy(), g["image_pooled"]), "text_pooled": rel_l2(pt.numpy(), g["text_pooled"]),
            "image_tokens_rows": rel_l2(ti.numpy()[:, ROWS_V], g["image_tokens_rows"]),
            "text_tokens_rows": rel_l2(tt.numpy()[:, ROWS_T], g["text_tokens_rows"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", nargs="+", default=["f32:8", "f32:16", "f64:8"], help="dtype:threads")
    ap.add_argument("--items", type=int, default=40)
    ap.add_argument("--kinds", nargs="+", default=KINDS)
    ap.add_argument("--parity", action="store_true")
    a = ap.parse_args()
    cfg = get_model_config("ViT-L-14-336")
    sd = W.synthetic_state_dict(cfg)
    heads_np = W.synthetic_pacl_heads(cfg.with_pacl(768))
    for run in a.runs:
        dt, th = run.split(":")
        dtype = torch.float64 if dt == "f64" else torch.float32
        torch.set_num_threads(int(th))
        o = Oracle(sd, cfg, dtype)
        heads = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in heads_np.items()}
        t0 = time.time()
        if a.parity:
            print(json.dumps({"run": run, "rel_l2": run_parity(o), "s": round(time.time() - t0, 1)}), flush=True)
            continue
        with torch.inference_mode():
            res = run_kinds(o, heads, a.kinds, a.items)
        gap = res.pop("_sigma_gap", {})
        for kind, (m, ref) in res.items():
            d = np.abs(m - ref)
            rec = {"run": run, "kind": kind, "items": int(d.size), "max_abs_diff": float(d.max()), "argmax": int(d.argmax()),
                   "min_abs_ref_margin": float(np.abs(ref).min()), "decisions_same": int(((m > 0) == (ref > 0)).sum())}
            if kind in gap:
                rec["min_weight_minus_sigma"] = float(np.nanmin(gap[kind]))
            print(json.dumps(rec), flush=True)
        print(json.dumps({"run": run, "s": round(time.time() - t0, 1)}), flush=True)


if __name__ == "__main__":
    main()
