#!/usr/bin/env python3
"""PyTorch state_dict -> MIUNETW1 weight file.

The reference's model chain (.pt -> .onnx -> .trt) is unpublished (/root/reference/.gitignore:2-8); this is the importer a
user of the reference needs to bring their own trained UNet.  Accepted key layout = the common Pytorch-UNet module tree
    inc.double_conv.{0,3}.weight / {1,4}.{weight,bias,running_mean,running_var}
    down{i}.maxpool_conv.1.double_conv....            (i = 1..levels)
    up{i}.up.{weight,bias}, up{i}.conv.double_conv....   (bilinear=False: transposed 2x2 upsampling)
    up{i}.conv.double_conv....                          (bilinear=True: no up{i}.up tensors -> a version 2 file)
    outc.conv.{weight,bias}
(conv biases, if present, are folded into the BatchNorm mean: BN(x + b) == BN'(x) with mean' = mean - b).  The variant is
detected from the keys and every tensor's shape is checked against miunet/spec.py's topology before anything is written.

    python tools/import_state_dict.py model.pt out.miw [--bn-eps 1e-5]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unet-medical-image-contour-segmentation-cpp_amd"))
from miunet.spec import UNetSpec, pack_weights  # noqa: E402


def _first_problem(spec: UNetSpec, t: dict):
    """The first tensor of `spec` that `t` lacks or holds in another shape, as a message; None when all match."""
    for name, shape in spec.tensor_list():
        if name not in t:
            return f"missing {name}"
        if tuple(t[name].shape) != tuple(shape):
            return f"{name}: shape {tuple(t[name].shape)}, the {spec.up} topology needs {tuple(shape)}"
    return None


def convert(sd: dict, bn_eps: float = 1e-5):
    """sd: name -> array-like.  Returns (spec, weight-file bytes): version 1 for a transposed-conv decoder, version 2 for a
    bilinear one (Pytorch-UNet bilinear=True).  A state dict that is neither raises ValueError naming the first missing or
    misshapen key."""
    g = {k: np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float32) for k, v in sd.items()
         if not k.endswith("num_batches_tracked")}
    for key in ("inc.double_conv.0.weight", "outc.conv.weight", "down1.maxpool_conv.1.double_conv.0.weight"):
        if key not in g:
            raise ValueError(f"not a Pytorch-UNet state dict: missing {key}")
    levels = 0
    while f"down{levels + 1}.maxpool_conv.1.double_conv.0.weight" in g:
        levels += 1
    if "up1.up.weight" in g:
        up = "transpose"
    elif "up1.conv.double_conv.0.weight" in g:
        up = "bilinear"
    else:
        raise ValueError("not a Pytorch-UNet state dict: missing up1.up.weight (transposed) and up1.conv.double_conv.0.weight (bilinear)")
    w0 = g["inc.double_conv.0.weight"]
    spec = UNetSpec(in_ch=int(w0.shape[1]), base=int(w0.shape[0]), levels=levels, classes=int(g["outc.conv.weight"].shape[0]),
                    bn_eps=bn_eps, up=up)
    t = {}

    def take(key):
        if key not in g:
            raise ValueError(f"{spec.up} Pytorch-UNet state dict: missing {key}")
        return g[key]

    def dconv(src, dst):
        for k, (ci, bi) in enumerate(((0, 1), (3, 4)), start=1):
            t[f"{dst}.c{k}.w"] = take(f"{src}.{ci}.weight")
            mean = take(f"{src}.{bi}.running_mean").copy()
            if f"{src}.{ci}.bias" in g:
                mean = mean - g[f"{src}.{ci}.bias"]
            t[f"{dst}.bn{k}.gamma"] = take(f"{src}.{bi}.weight")
            t[f"{dst}.bn{k}.beta"] = take(f"{src}.{bi}.bias")
            t[f"{dst}.bn{k}.mean"] = mean
            t[f"{dst}.bn{k}.var"] = take(f"{src}.{bi}.running_var")

    dconv("inc.double_conv", "inc")
    for i in range(1, levels + 1):
        dconv(f"down{i}.maxpool_conv.1.double_conv", f"down{i}")
        if up == "transpose":
            t[f"up{i}.t.w"] = take(f"up{i}.up.weight")
            t[f"up{i}.t.b"] = take(f"up{i}.up.bias")
        dconv(f"up{i}.conv.double_conv", f"up{i}")
    ow = take("outc.conv.weight")
    t["outc.w"] = ow.reshape(ow.shape[0], -1)
    t["outc.b"] = take("outc.conv.bias")
    problem = _first_problem(spec, t)
    if problem:
        raise ValueError(f"{spec.up} Pytorch-UNet state dict (in_ch={spec.in_ch} base={spec.base} levels={levels}): {problem}")
    return spec, pack_weights(spec, t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("state_dict")
    ap.add_argument("out")
    ap.add_argument("--bn-eps", type=float, default=1e-5)
    a = ap.parse_args()
    import torch

    sd = torch.load(a.state_dict, map_location="cpu")
    if isinstance(sd, dict) and "state_dict" in sd:
        sd = sd["state_dict"]
    spec, blob = convert(sd, a.bn_eps)
    open(a.out, "wb").write(blob)
    print(f"wrote {a.out}: in_ch={spec.in_ch} base={spec.base} levels={spec.levels} classes={spec.classes} upsample={spec.up} "
          f"({len(blob)} bytes)")


if __name__ == "__main__":
    main()
