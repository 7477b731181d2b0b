"""Generator for the model / dataset yaml config surface.

The reference describes its two-stream networks with `models/transformer/*_Transfusion_*.yaml` files (schema:
nc, depth_multiple, width_multiple, anchors, backbone, head — each layer a `[from, number, module, args]` row,
consumed by parse_model, reference models/yolo_test.py:216-302) and its datasets with
`data/multispectral/*.yaml` (schema: path, train_rgb, val_rgb, train_ir, val_ir, nc, names — reference
data/multispectral/kaist.yaml:13-23).  All twelve Transfusion files differ only in (nc, depth_multiple,
width_multiple), so they are emitted from one description here; `python -m icafusion_amd.configs` rewrites the
yaml files in the repo.  An optional trailing `{loops_num: n}` mapping in a TransformerFusionBlock row exposes the
parameter-shared iteration count that the reference wires (models/common.py:691,744) but never surfaces in a yaml; the
positional arguments keep the reference's meaning (a 4th positional would be `h`, the number of heads).
"""
import os
import yaml

SIZES = {"n": (0.33, 0.25), "s": (0.33, 0.50), "m": (0.67, 0.75), "l": (1.0, 1.0)}
ANCHORS = [[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119], [116, 90, 156, 198, 373, 326]]
# (size letter, dataset tag, nc) — the Transfusion variants the reference ships
VARIANTS = [("l", "FLIR", 3), ("l", "LLVIP", 1), ("l", "VEDAI", 9), ("l", "kaist", 1),
            ("m", "FLIR", 3), ("m", "SeaDrone", 7), ("m", "VEDAI", 9), ("m", "kaist", 1),
            ("n", "FLIR", 3), ("n", "kaist", 1), ("s", "FLIR", 3), ("s", "kaist", 1)]
TOKENS = ((20, 20), (16, 16), (10, 10))   # (vert_anchors, horz_anchors) for P3, P4, P5
# the simpler fusion blocks the reference ships on the same two-stream backbone
FUSION_VARIANTS = [("l", "NiNfusion", "FLIR", 3), ("l", "NiNfusion", "LLVIP", 1), ("l", "NiNfusion", "VEDAI", 9),
                   ("m", "NiNfusion", "FLIR", 3), ("m", "NiNfusion", "kaist", 1), ("n", "NiNfusion", "FLIR", 3),
                   ("l", "Add", "FLIR", 3), ("m", "Add", "kaist", 1), ("n", "Add", "kaist", 1), ("s", "Add", "kaist", 1)]

DATASETS = {
    "kaist": (1, ["person"]), "LLVIP": (1, ["person"]), "CVC14": (1, ["person"]), "FLIR-align": (1, ["person"]),
    "FLIR-align-3class": (3, ["person", "car", "bicycle"]),
    "VEDAI": (9, ["car", "truck", "pickup", "tractor", "camper", "ship", "van", "plane", "other"]),
}


def _stream(first_from):
    """One CSPDarknet stream (10 layers); the IR stream starts with from=-4 meaning 'take the second input'."""
    widths, repeats = (128, 256, 512, 1024), (3, 6, 9, 3)
    rows = [[first_from, 1, "Conv", [64, 6, 2, 2]]]
    for w, r in zip(widths, repeats):
        rows.append([-1, 1, "Conv", [w, 3, 2]])
        rows.append([-1, r, "C3", [w]])
    rows.append([-1, 1, "SPPF", [1024, 5]])
    return rows


def transfusion_cfg(size="s", nc=1, loops=1, fusion="TransformerFusionBlock"):
    """fusion: "TransformerFusionBlock" (DMFF), "NiNfusion" (concat + 1x1 conv + SiLU, models/common.py:348-360) or "Add"
    (weighted sum, :324-331)."""
    gd, gw = SIZES[size]
    backbone = _stream(-1) + _stream(-4)
    taps = ((4, 14, 256), (6, 16, 512), (9, 19, 1024))
    for (a, b, c), (va, ha) in zip(taps, TOKENS):
        if fusion == "NiNfusion":
            backbone.append([[a, b], 1, "NiNfusion", [1, 1]])
            continue
        if fusion == "Add":
            backbone.append([[a, b], 1, "Add", [1]])
            continue
        args = [c, va, ha] + ([{"loops_num": loops}] if loops != 1 else [])
        backbone.append([[a, b], 1, "TransformerFusionBlock", args])
    head = [
        [-1, 1, "Conv", [512, 1, 1]], [-1, 1, "nn.Upsample", ["None", 2, "nearest"]], [[-1, 21], 1, "Concat", [1]],
        [-1, 3, "C3", [512, False]],
        [-1, 1, "Conv", [256, 1, 1]], [-1, 1, "nn.Upsample", ["None", 2, "nearest"]], [[-1, 20], 1, "Concat", [1]],
        [-1, 3, "C3", [256, False]],
        [-1, 1, "Conv", [256, 3, 2]], [[-1, 27], 1, "Concat", [1]], [-1, 3, "C3", [512, False]],
        [-1, 1, "Conv", [512, 3, 2]], [[-1, 23], 1, "Concat", [1]], [-1, 3, "C3", [1024, False]],
        [[30, 33, 36], 1, "Detect", ["nc", "anchors"]],
    ]
    return {"nc": nc, "depth_multiple": gd, "width_multiple": gw, "anchors": [list(a) for a in ANCHORS],
            "backbone": backbone, "head": head}


# (fusion block, dataset tag, nc) — the VGG16-backbone variants the reference ships
VGG16_VARIANTS = [("Transfusion", "kaist", 1), ("Transfusion", "FLIR", 3), ("NiNfusion", "kaist", 1), ("NiNfusion", "FLIR", 3)]
VGG16_BLOCKS = ((2, 3, 64), (2, 64, 128), (3, 128, 256), (3, 256, 512), (3, 512, 512))     # (num_convs, c1, c2), each closed by a 2x2 pool
VGG16_TAPS = ((2, 7, 256), (3, 8, 512), (4, 9, 512))                                      # (RGB row, IR row, channels) at strides 8, 16, 32


def vgg16_cfg(fusion="Transfusion", nc=1):
    """Two VGG16 streams (five VGGblock rows each, models/common.py:109-128), DMFF ("Transfusion") or NiNfusion taps behind blocks 3, 4 and
    5, and the yolov5l PANet head on 512 / 512 / 256 channels."""
    backbone = [[f if i == 0 else -1, 1, "VGGblock", list(b)] for f in (-1, -4) for i, b in enumerate(VGG16_BLOCKS)]
    for (a, b, c), (va, ha) in zip(VGG16_TAPS, TOKENS):
        backbone.append([[a, b], 1, "NiNfusion", [1, 1]] if fusion == "NiNfusion" else [[a, b], 1, "TransformerFusionBlock", [c, va, ha]])
    head = [
        [-1, 1, "Conv", [512, 1, 1]], [-1, 1, "nn.Upsample", ["None", 2, "nearest"]], [[-1, 11], 1, "Concat", [1]],
        [-1, 3, "C3", [512, False]],
        [-1, 1, "Conv", [256, 1, 1]], [-1, 1, "nn.Upsample", ["None", 2, "nearest"]], [[-1, 10], 1, "Concat", [1]],
        [-1, 3, "C3", [256, False]],
        [-1, 1, "Conv", [256, 3, 2]], [[-1, 17], 1, "Concat", [1]], [-1, 3, "C3", [512, False]],
        [-1, 1, "Conv", [512, 3, 2]], [[-1, 13], 1, "Concat", [1]], [-1, 3, "C3", [512, False]],
        [[20, 23, 26], 1, "Detect", ["nc", "anchors"]],
    ]
    return {"nc": nc, "depth_multiple": 1.0, "width_multiple": 1.0, "anchors": [list(a) for a in ANCHORS],
            "backbone": backbone, "head": head}


# (fusion block, dataset tag, nc) — the ResNet50-backbone variants the reference ships
RESNET50_VARIANTS = [("Transfusion", "kaist", 1), ("Transfusion", "FLIR", 3), ("NiNfusion", "kaist", 1), ("NiNfusion", "FLIR", 3)]
# (c1, c2, stride, is_first, num_blocks) as the reference writes them: the 7x7 stem row, then 3-4-6-3 bottleneck blocks ending on 4 * c2 channels
RESNET50_ROWS = ((3, 64, 1, True, 1), (64, 64, 1, False, 3), (256, 128, 2, False, 4), (512, 256, 2, False, 6), (1024, 512, 2, False, 3))
RESNET50_TAPS = ((2, 7, 512), (3, 8, 1024), (4, 9, 2048))                                 # (RGB row, IR row, channels) at strides 8, 16, 32


def resnet50_cfg(fusion="Transfusion", nc=1):
    """Two ResNet50 streams (five ResNetlayer rows each, models/common.py:131-181), DMFF ("Transfusion") or NiNfusion taps behind rows 2, 3
    and 4 (C = 512 / 1024 / 2048), and a PANet head on the reference's widths 1024 / 512 / 512 / 1024 / 1024 / 2048."""
    backbone = [[f if i == 0 else -1, 1, "ResNetlayer", list(r)] for f in (-1, -4) for i, r in enumerate(RESNET50_ROWS)]
    for (a, b, c), (va, ha) in zip(RESNET50_TAPS, TOKENS):
        backbone.append([[a, b], 1, "NiNfusion", [1, 1]] if fusion == "NiNfusion" else [[a, b], 1, "TransformerFusionBlock", [c, va, ha]])
    head = [
        [-1, 1, "Conv", [1024, 1, 1]], [-1, 1, "nn.Upsample", ["None", 2, "nearest"]], [[-1, 11], 1, "Concat", [1]],
        [-1, 3, "C3", [1024, False]],
        [-1, 1, "Conv", [512, 1, 1]], [-1, 1, "nn.Upsample", ["None", 2, "nearest"]], [[-1, 10], 1, "Concat", [1]],
        [-1, 3, "C3", [512, False]],
        [-1, 1, "Conv", [512, 3, 2]], [[-1, 17], 1, "Concat", [1]], [-1, 3, "C3", [1024, False]],
        [-1, 1, "Conv", [1024, 3, 2]], [[-1, 13], 1, "Concat", [1]], [-1, 3, "C3", [2048, False]],
        [[20, 23, 26], 1, "Detect", ["nc", "anchors"]],
    ]
    return {"nc": nc, "depth_multiple": 1.0, "width_multiple": 1.0, "anchors": [list(a) for a in ANCHORS],
            "backbone": backbone, "head": head}


def _dump_model_yaml(cfg, title, streams="CSPDarknet", fusion="Transfusion"):
    """fusion: what the header says the three taps are — the files written before the ResNet50 ones keep the DMFF wording whatever they fuse with"""
    taps = {"Transfusion": ("three DMFF", "# (TransformerFusionBlock)"), "NiNfusion": ("three NiNfusion", "# (concatenate + 1x1 Conv)")}[fusion]
    lines = [f"# {title}", f"# generated by icafusion_amd/configs.py — two RGB/IR {streams} streams, {taps[0]}",
             f"{taps[1]} taps at P3/P4/P5, PANet head, Detect.  Row = [from, number, module, args];",
             "# from=-4 feeds the IR image; optional trailing {loops_num: n} DMFF arg = number of parameter-shared iterations.",
             f"nc: {cfg['nc']}", f"depth_multiple: {cfg['depth_multiple']}", f"width_multiple: {cfg['width_multiple']}",
             "anchors:"]
    lines += [f"  - {a}" for a in cfg["anchors"]]
    for sec in ("backbone", "head"):
        lines.append(f"{sec}:")
        base = 0 if sec == "backbone" else len(cfg["backbone"])
        for i, row in enumerate(cfg[sec]):
            txt = yaml.safe_dump(row, default_flow_style=True, width=200).strip()
            lines.append(f"  - {txt}  # {base + i}")
    return "\n".join(lines) + "\n"


def write_all(root):
    os.makedirs(os.path.join(root, "models", "transformer"), exist_ok=True)
    os.makedirs(os.path.join(root, "data", "multispectral"), exist_ok=True)
    for size, tag, nc in VARIANTS:
        name = f"yolov5{size}_Transfusion_{tag}.yaml"
        with open(os.path.join(root, "models", "transformer", name), "w") as f:
            f.write(_dump_model_yaml(transfusion_cfg(size, nc), name))
    with open(os.path.join(root, "models", "transformer", "yolov5s_Transfusion_kaist_loops3.yaml"), "w") as f:
        f.write(_dump_model_yaml(transfusion_cfg("s", 1, loops=3), "yolov5s + DMFF, 3 shared-weight iterations"))
    for size, fusion, tag, nc in FUSION_VARIANTS:
        name = f"yolov5{size}_{fusion}_{tag}.yaml"
        with open(os.path.join(root, "models", "transformer", name), "w") as f:
            f.write(_dump_model_yaml(transfusion_cfg(size, nc, fusion=fusion), name))
    for fusion, tag, nc in VGG16_VARIANTS:
        name = f"yolov5_VGG16_{fusion}_{tag}.yaml"
        with open(os.path.join(root, "models", "transformer", name), "w") as f:
            f.write(_dump_model_yaml(vgg16_cfg(fusion, nc), name, streams="VGG16"))
    for fusion, tag, nc in RESNET50_VARIANTS:
        name = f"yolov5_ResNet50_{fusion}_{tag}.yaml"
        with open(os.path.join(root, "models", "transformer", name), "w") as f:
            f.write(_dump_model_yaml(resnet50_cfg(fusion, nc), name, streams="ResNet50", fusion=fusion))
    for tag, (nc, names) in DATASETS.items():
        d = f"/data/{tag}"
        body = {"path": d, "train_rgb": f"{d}/visible/train/", "val_rgb": f"{d}/visible/test/",
                "train_ir": f"{d}/infrared/train/", "val_ir": f"{d}/infrared/test/", "nc": nc, "names": names}
        with open(os.path.join(root, "data", "multispectral", f"{tag}.yaml"), "w") as f:
            f.write(f"# paired RGB / IR dataset descriptor ({tag}); edit the paths for your machine\n")
            f.write(yaml.safe_dump(body, sort_keys=False, default_flow_style=None))


if __name__ == "__main__":
    write_all(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
