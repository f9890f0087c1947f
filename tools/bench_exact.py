"""Speed of the fp32 precision mode on one GPU, beside the default bf16 path: ms per encode_image
(B = 1, 2, 16) and encode_text (B = 2) at full depth, ce_kernel_stats per tag of one B = 2 call in
fp32 mode, and the f32 GEMM alone (ce_kernel_gemm_f32, bias + GELU) on c_fc of one image (M = 577),
of 16 images, and on 4096^3.  Three warm-up calls, then five rounds of repeated calls on a host clock
that ends in a device synchronise; median, minimum and maximum of the rounds.

    python tools/bench_exact.py [--out FILE.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "clip-embeds_amd"), REPO]
import clipembed  # noqa: E402
from clipembed import _lib, weights as W  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the JSON here")
args = ap.parse_args()
dev = torch.device("cuda", 0)
cfg = clipembed.get_model_config("ViT-L-14-336")
sd = W.synthetic_state_dict(cfg)
out = {}


def timeit(fn, reps, rounds=5):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / reps * 1e3)
    return {"ms_median": sorted(ts)[len(ts) // 2], "ms_min": min(ts), "ms_max": max(ts)}


for prec in ("fp32", "bf16"):
    m = clipembed.CLIP(cfg)
    m.set_precision(prec)
    m.load_state_dict(sd)
    m.to(dev)
    free0 = torch.cuda.mem_get_info()[0]
    for B in (1, 2, 16):
        imgs = torch.from_numpy(W.synthetic_images(B, seed=1000)).to(dev)
        out[f"{prec}_encode_image_B{B}"] = timeit(lambda: m.encode_image(imgs), 10)
    caps = torch.from_numpy(W.synthetic_captions(2, seed=2000)).to(dev)
    out[f"{prec}_encode_text_B2"] = timeit(lambda: m.encode_text(caps), 20)
    if prec == "fp32":
        imgs = torch.from_numpy(W.synthetic_images(2, seed=1000)).to(dev)
        m.engine.set_timing(True)
        for _ in range(5):
            m.encode_image(imgs)
            m.encode_text(caps)
        torch.cuda.synchronize()
        st = m.engine.kernel_stats()
        m.engine.set_timing(False)
        out["fp32_kernel_stats_B2_per_call"] = {
            k["name"]: {"ms": k["ms"] / 5, "launches": k["launches"] // 5,
                        "tflops": (k["flops"] / (k["ms"] * 1e-3) / 1e12) if k["ms"] > 0 and k["flops"] > 0 else None}
            for k in st}
    del m
    torch.cuda.empty_cache()

# the f32 GEMM alone
P = lambda t: ctypes.c_void_p(t.data_ptr())
S = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
for M in (577, 16 * 577, 4096):
    N, K = (4096, 1024) if M != 4096 else (4096, 4096)
    A = torch.randn(M, K, device=dev)
    Wt = torch.randn(N, K, device=dev) * K ** -0.5
    bias = torch.randn(N, device=dev)
    o = torch.empty(M, N, device=dev)
    r = timeit(lambda: _lib.call("ce_kernel_gemm_f32", S(), P(A), K, P(Wt), M, N, K, P(bias), 1, None, P(o), N), 50)
    r["tflops_median"] = 2.0 * M * N * K / (r["ms_median"] * 1e-3) / 1e12
    out[f"gemm_f32_{M}x{N}x{K}_gelu"] = r

if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
print(json.dumps(out, indent=1))
