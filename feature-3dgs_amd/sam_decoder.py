"""SAM's prompt encoder and mask decoder on the device: from a rendered 256-channel feature map and point / box prompts to the
decoder's low-resolution logits and IoU predictions - the step between the rasterizer's feature map and sam_masks.py.

Replaces what the reference runs between `SamPredictor.set_image(..., features=...)` and `postprocess_masks`
(encoders/sam_encoder/segment_anything/predictor.py:predict_torch) -

    sparse, dense = model.prompt_encoder(points=(coords, labels), boxes=boxes, masks=None)
    low_res, iou = model.mask_decoder(image_embeddings=features, image_pe=model.prompt_encoder.get_dense_pe(),
                                      sparse_prompt_embeddings=sparse, dense_prompt_embeddings=dense, multimask_output=...)

- with

    weights = SamDecoderWeights.from_state_dict(torch.load("sam_vit_h.pth"))        # any dict with the reference's names
    p = plan(weights, features)                                                     # once per feature map (256, h, w)
    low_res, iou = predict(p, point_coords, point_labels, boxes=None, multimask_output=True)
    predictor = SamFeaturePredictor(weights);  predictor.set_image((H, W), features=features);  predictor.predict_torch(...)
    records = generate(weights, features, (H, W), points_per_side=32, points_per_batch=64, pred_iou_thresh=0.88)

csrc/sam_decoder.hip behind include/f3dgs.h (f3dgs_sam_decoder_*).  Exactly SAM's decoder (width 256, depth 2, 8 heads, MLP
2048, 4 mask tokens + 1 IoU token); other architectures and the mask prompt raise NotImplementedError.  fp32 throughout, every
contraction on the exact-fp32 matrix instructions, every reduction in a fixed order: two calls give the same bits, and a
prompt's outputs are the same bits at every batch size and every position in the batch.  The image encoder (ViT) is not part of
this project: the features are the rendered ones.  Neither `segment_anything` nor torchvision is imported.

HIP only; no CPU fallback; argument errors are raised before any device work.
"""
from __future__ import annotations

import numpy as np
import torch

from sam_masks import MaskPostprocessor, upscale_masks

DIM = 256
MAX_TOKENS = 16                 # F3DGS_SAM_DECODER_MAX_TOKENS: 5 output tokens + prompt tokens
MAX_GRID = 16384                # F3DGS_SAM_DECODER_MAX_GRID: cells of the embedding grid
MAX_PROMPTS = 65535             # per predict call


def _attention(prefix, inner):
    return [(f"{prefix}.q_proj.weight", (inner, DIM)), (f"{prefix}.q_proj.bias", (inner,)),
            (f"{prefix}.k_proj.weight", (inner, DIM)), (f"{prefix}.k_proj.bias", (inner,)),
            (f"{prefix}.v_proj.weight", (inner, DIM)), (f"{prefix}.v_proj.bias", (inner,)),
            (f"{prefix}.out_proj.weight", (DIM, inner)), (f"{prefix}.out_proj.bias", (DIM,))]


def _module(prefix, *shape):
    return [(f"{prefix}.weight", tuple(shape)), (f"{prefix}.bias", (shape[0],))]


def parameter_table():
    """[(name, shape)]: the reference's parameters in the order f3dgs_sam_decoder_pack_weights takes them (include/f3dgs.h)."""
    t = [("prompt_encoder.pe_layer.positional_encoding_gaussian_matrix", (2, DIM // 2))]
    t += [(f"prompt_encoder.point_embeddings.{i}.weight", (1, DIM)) for i in range(4)]
    t += [("prompt_encoder.not_a_point_embed.weight", (1, DIM)), ("prompt_encoder.no_mask_embed.weight", (1, DIM)),
          ("mask_decoder.iou_token.weight", (1, DIM)), ("mask_decoder.mask_tokens.weight", (4, DIM))]
    for l in range(2):
        p = f"mask_decoder.transformer.layers.{l}"
        t += _attention(f"{p}.self_attn", DIM) + _module(f"{p}.norm1", DIM)
        t += _attention(f"{p}.cross_attn_token_to_image", DIM // 2) + _module(f"{p}.norm2", DIM)
        t += _module(f"{p}.mlp.lin1", 2048, DIM) + _module(f"{p}.mlp.lin2", DIM, 2048)
        t += _module(f"{p}.norm3", DIM) + _module(f"{p}.norm4", DIM)
        t += _attention(f"{p}.cross_attn_image_to_token", DIM // 2)
    t += _attention("mask_decoder.transformer.final_attn_token_to_image", DIM // 2) + _module("mask_decoder.transformer.norm_final_attn", DIM)
    t += [("mask_decoder.output_upscaling.0.weight", (DIM, 64, 2, 2)), ("mask_decoder.output_upscaling.0.bias", (64,))]
    t += _module("mask_decoder.output_upscaling.1", 64)
    t += [("mask_decoder.output_upscaling.3.weight", (64, 32, 2, 2)), ("mask_decoder.output_upscaling.3.bias", (32,))]
    for i in range(4):
        p = f"mask_decoder.output_hypernetworks_mlps.{i}.layers"
        t += _module(f"{p}.0", DIM, DIM) + _module(f"{p}.1", DIM, DIM) + _module(f"{p}.2", 32, DIM)
    p = "mask_decoder.iou_prediction_head.layers"
    t += _module(f"{p}.0", DIM, DIM) + _module(f"{p}.1", DIM, DIM) + _module(f"{p}.2", 4, DIM)
    return t


def _C():
    from diff_gaussian_rasterization import _C as ext
    return ext


def _device(device):
    """The HIP device the weights go to; the refusal without one."""
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("sam_decoder needs a HIP device: there is no CPU path")
        return torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"sam_decoder needs a HIP device, got {device}: there is no CPU path")
    return device


class SamDecoderWeights:
    """The packed parameters of the prompt encoder and the mask decoder on one device (16 MB)."""

    def __init__(self, packed):
        self.packed = packed

    @property
    def device(self):
        return self.packed.device

    @classmethod
    def from_state_dict(cls, sd, prefix="", device=None):
        """sd: a SAM checkpoint's state dict, or any dict that has the reference's names under `prefix + "prompt_encoder."` and
        `prefix + "mask_decoder."` (the image encoder's entries and the mask prompt's `mask_downscaling` are ignored).  A missing
        name raises KeyError, a wrong shape ValueError - or NotImplementedError where the shape is another architecture's
        (another width, depth or number of mask tokens); each names the parameter.  Then the refusal without a HIP device."""
        tensors = []
        if f"{prefix}mask_decoder.transformer.layers.2.norm1.weight" in sd:
            raise NotImplementedError(f"{prefix}mask_decoder.transformer.layers.2: a transformer of depth 2 is built, this one is deeper")
        for name, shape in parameter_table():
            key = prefix + name
            if key not in sd:
                raise KeyError(f"{key}: not in the state dict")
            t = torch.as_tensor(sd[key])
            if tuple(t.shape) != shape:
                if t.dim() == len(shape):
                    raise NotImplementedError(f"{key}: shape {tuple(t.shape)}, SAM's decoder (width {DIM}, 8 heads, MLP 2048, 4 mask tokens) "
                                              f"has {shape}: other architectures are not built")
                raise ValueError(f"{key}: shape {tuple(t.shape)}, {shape} expected")
            if not t.dtype.is_floating_point:
                raise ValueError(f"{key}: a floating-point tensor expected, got {t.dtype}")
            tensors.append(t)
        device = _device(device)
        params = [t.detach().to(device=device, dtype=torch.float32).contiguous() for t in tensors]
        return cls(_C().sam_decoder_pack(params))


class SamImagePlan:
    """What is the same for every prompt of one feature map: the token-major embedding, the dense positional encoding and layer
    0's projections of the image tokens (3584 bytes per cell)."""

    def __init__(self, weights, data, grid):
        self.weights, self.data, self.grid = weights, data, grid


@torch.no_grad()
def plan(weights, features) -> SamImagePlan:
    """features: float32 (256, h, w) or (1, 256, h, w) on the weights' device, h w <= 16384; any strides - a view of a larger
    rendered tensor is read in place and gives the bits of its contiguous copy."""
    if not isinstance(weights, SamDecoderWeights):
        raise ValueError("weights: SamDecoderWeights expected")
    if not torch.is_tensor(features) or features.dtype != torch.float32:
        raise ValueError("features: a float32 tensor (256, h, w) expected")
    if features.dim() == 4 and features.shape[0] == 1:
        features = features[0]
    if features.dim() != 3 or features.shape[1] < 1 or features.shape[2] < 1:
        raise ValueError(f"features: (256, h, w) expected, got {tuple(features.shape)}")
    if features.shape[0] != DIM:
        raise NotImplementedError(f"features of {features.shape[0]} channels: SAM's decoder has {DIM}, other widths are not built")
    h, w = int(features.shape[1]), int(features.shape[2])
    if h * w > MAX_GRID:
        raise NotImplementedError(f"a {h} x {w} embedding grid: up to {MAX_GRID} cells are built")
    if features.device != weights.device:
        raise ValueError(f"features live on {features.device}, the weights on {weights.device} (no CPU path)")
    return SamImagePlan(weights, _C().sam_decoder_plan(weights.packed, features.detach()), (h, w))


def _prompts(point_coords, point_labels, boxes, device):
    """(coords (B,n,2) float32, labels (B,n) int32, boxes (B,4) float32 or None), checked; NotImplementedError beyond 16 tokens."""
    if point_coords is None and boxes is None:
        raise ValueError("neither points nor boxes: a prompt needs one of them")
    if (point_coords is None) != (point_labels is None):
        raise ValueError("point_coords and point_labels go together")
    B = None
    if boxes is not None:
        boxes = torch.as_tensor(boxes)
        if boxes.dim() == 3 and boxes.shape[1:] == (1, 4):
            boxes = boxes[:, 0]
        if boxes.dim() != 2 or boxes.shape[1] != 4:
            raise ValueError(f"boxes: (B, 4) XYXY expected, got {tuple(boxes.shape)}")
        B = boxes.shape[0]
    if point_coords is not None:
        point_coords, point_labels = torch.as_tensor(point_coords), torch.as_tensor(point_labels)
        if point_coords.dim() != 3 or point_coords.shape[2] != 2:
            raise ValueError(f"point_coords: (B, n, 2) expected, got {tuple(point_coords.shape)}")
        if tuple(point_labels.shape) != tuple(point_coords.shape[:2]):
            raise ValueError(f"point_labels: {tuple(point_coords.shape[:2])} expected, got {tuple(point_labels.shape)}")
        if B is not None and point_coords.shape[0] != B:
            raise ValueError(f"{point_coords.shape[0]} point prompts and {B} boxes")
        B, n = point_coords.shape[0], point_coords.shape[1]
    else:
        n = 0
    T = 5 + n + (2 if boxes is not None else 1)
    if T > MAX_TOKENS:
        raise NotImplementedError(f"{T} tokens per prompt (5 output tokens, {n} points, {'2 box corners' if boxes is not None else '1 pad point'}): "
                                  f"up to {MAX_TOKENS} are built")
    if B > MAX_PROMPTS:
        raise NotImplementedError(f"{B} prompts in one call: up to {MAX_PROMPTS} are built")
    if point_coords is None:
        point_coords = torch.zeros((B, 0, 2), dtype=torch.float32, device=device)
        point_labels = torch.zeros((B, 0), dtype=torch.int32, device=device)
    for name, t in (("point_coords", point_coords), ("point_labels", point_labels), ("boxes", boxes)):
        if t is not None and t.device != device:
            raise ValueError(f"{name} lives on {t.device}, the plan on {device} (no CPU path)")
    coords = point_coords.detach().to(torch.float32).contiguous()
    labels = point_labels.detach().to(torch.int32).contiguous()
    boxes = None if boxes is None else boxes.detach().to(torch.float32).contiguous()
    return coords, labels, boxes


@torch.no_grad()
def predict(plan, point_coords, point_labels, boxes=None, multimask_output=True, input_size=None, mask_input=None):
    """(low_res (B, m, 4h, 4w), iou_predictions (B, m)) float32, m = 3 (masks 1..3) with multimask_output, else 1 (mask 0): what
    predict_torch gets from the decoder before postprocess_masks.  point_coords (B, n, 2) (x, y) in pixels of the input image
    (already transformed to it, as for predict_torch), point_labels (B, n): 1 foreground, 0 background, -1 not a point; boxes
    (B, 4) XYXY or None.  input_size (height, width) of the input image, by default SAM's 1024 x 1024.  B = 0 gives empty
    tensors."""
    if not isinstance(plan, SamImagePlan):
        raise ValueError("plan: the SamImagePlan of plan() expected")
    if mask_input is not None:
        raise NotImplementedError("mask_input: the mask prompt (mask_downscaling) is not built; the dense prompt is no_mask_embed")
    ih, iw = (1024, 1024) if input_size is None else (int(input_size[0]), int(input_size[1]))
    if ih < 1 or iw < 1:
        raise ValueError(f"input_size {input_size!r}: (height, width) >= 1 expected")
    coords, labels, boxes = _prompts(point_coords, point_labels, boxes, plan.data.device)
    h, w = plan.grid
    return _C().sam_decoder_predict(plan.data, plan.weights.packed, h, w, coords, labels, boxes, ih, iw, bool(multimask_output))


class SamFeaturePredictor:
    """The drop-in for the reference's modified SamPredictor on rendered features.  `img_size` is the image encoder's (the side
    of the padded square the prompts and postprocess_masks refer to), 1024 for every SAM."""

    mask_threshold = 0.0

    def __init__(self, weights, img_size=1024):
        if not isinstance(weights, SamDecoderWeights):
            raise ValueError("weights: SamDecoderWeights expected (SamDecoderWeights.from_state_dict)")
        self.weights, self.img_size = weights, int(img_size)
        self.reset_image()

    @property
    def device(self):
        return self.weights.device

    def set_image(self, image_or_size, image_format="RGB", features=None):
        """image_or_size: the (H, W, 3) image or just its (H, W) - only the size is used.  features (256, h, w) or (1, 256, h, w)
        is REQUIRED: the image encoder is not built in this project, the features are the rendered ones."""
        if features is None:
            raise NotImplementedError("set_image without features: the image encoder (ViT) is not built in this project; pass the "
                                      "rendered feature map as features=")
        shape = tuple(image_or_size.shape[:2]) if hasattr(image_or_size, "shape") else tuple(int(v) for v in image_or_size)
        if len(shape) != 2 or min(shape) < 1:
            raise ValueError(f"image_or_size {image_or_size!r}: an image (H, W, 3) or its (H, W) expected")
        self.reset_image()
        self.original_size = shape
        scale = self.img_size / max(shape)                       # ResizeLongestSide.get_preprocess_shape
        self.input_size = (int(shape[0] * scale + 0.5), int(shape[1] * scale + 0.5))
        self.plan = plan(self.weights, features)
        self.features = features if features.dim() == 4 else features[None]
        self.is_image_set = True

    def predict_torch(self, point_coords, point_labels, boxes=None, mask_input=None, multimask_output=True, return_logits=False):
        """(masks (B, m, H, W), iou_predictions (B, m), low_res_masks (B, m, 4h, 4w)); the prompts are in the input frame (the
        image resized to img_size on its longest side), as for the reference's predict_torch."""
        if not self.is_image_set:
            raise RuntimeError("An image must be set with .set_image(...) before mask prediction.")
        low_res, iou = predict(self.plan, point_coords, point_labels, boxes, multimask_output, (self.img_size, self.img_size), mask_input)
        if low_res.shape[0] == 0:
            masks = torch.empty(tuple(low_res.shape[:2]) + self.original_size, dtype=torch.float32 if return_logits else torch.bool, device=low_res.device)
        else:
            masks = upscale_masks(low_res, self.img_size, self.input_size, self.original_size,
                                  out=torch.float32 if return_logits else torch.bool, mask_threshold=self.mask_threshold)
        return masks, iou, low_res

    def get_image_embedding(self):
        if not self.is_image_set:
            raise RuntimeError("An image must be set with .set_image(...) to generate an embedding.")
        return self.features

    def reset_image(self):
        self.is_image_set = False
        self.features = self.plan = self.original_size = self.input_size = None


def point_grid(n_per_side) -> np.ndarray:
    """utils/amg.py:build_point_grid: (n^2, 2) float64 points (x, y) in [0, 1]^2 at (i + 0.5) / n, x fastest."""
    n = int(n_per_side)
    if n < 1:
        raise ValueError(f"points_per_side {n_per_side!r}: an integer >= 1 expected")
    offset = 1 / (2 * n)
    side = np.linspace(offset, 1 - offset, n)
    return np.stack([np.tile(side[None, :], (n, 1)), np.tile(side[:, None], (1, n))], axis=-1).reshape(-1, 2)


@torch.no_grad()
def generate(weights, features, original_size, points_per_side=32, points_per_batch=64, img_size=1024, **postprocessor_kwargs) -> list:
    """SamAutomaticMaskGenerator.generate on rendered features, crop layer 0 only (the reference's feature route has no features
    for crops): the point grid scaled to the image, in batches of points_per_batch through predict (three masks per point) and
    MaskPostprocessor.add_batch, then finish().  postprocessor_kwargs: MaskPostprocessor's (pred_iou_thresh, ...)."""
    if "crop_n_layers" in postprocessor_kwargs:
        raise NotImplementedError("crop_n_layers: only crop layer 0 (the whole image) is built")
    if int(points_per_batch) < 1:
        raise ValueError(f"points_per_batch {points_per_batch!r}: an integer >= 1 expected")
    predictor = SamFeaturePredictor(weights, img_size)
    predictor.set_image(original_size, features=features)
    H, W = predictor.original_size
    pp = MaskPostprocessor((H, W), **postprocessor_kwargs)
    points = point_grid(points_per_side) * np.array([[W, H]], dtype=np.float64)
    ih, iw = predictor.input_size
    for at in range(0, points.shape[0], int(points_per_batch)):
        batch = points[at:at + int(points_per_batch)]
        # ResizeLongestSide.apply_coords: to the input frame, in float64, then float32 as the reference's as_tensor
        scaled = batch * np.array([[iw / W, ih / H]], dtype=np.float64)
        coords = torch.as_tensor(scaled, dtype=torch.float32, device=weights.device)[:, None, :]
        labels = torch.ones((coords.shape[0], 1), dtype=torch.int32, device=weights.device)
        low_res, iou = predict(predictor.plan, coords, labels, None, True, (img_size, img_size))
        pp.add_batch(low_res, iou, batch, (0, 0, W, H), predictor.input_size, predictor.original_size, img_size)
    return pp.finish()


def install(module):
    """Sets `SamPredictor` in an imported `segment_anything`-like module (or its `predictor` submodule) to SamFeaturePredictor, so
    that a caller of the reference who builds `SamPredictor(...)` with SamDecoderWeights runs on the fused kernels.  Returns the
    module."""
    if not hasattr(module, "SamPredictor"):
        raise AttributeError(f"{module.__name__} has no SamPredictor: not the reference's segment_anything")
    module.SamPredictor = SamFeaturePredictor
    return module
