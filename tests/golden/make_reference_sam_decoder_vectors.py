"""Generates tests/golden/reference_sam_decoder.npz (CASES) and tests/golden/reference_sam_decoder_edges.npz (EDGE_CASES: the tile,
chunk and grid-limit edges, each recorded as a sample - edge_sample_index) by running the reference's own prompt encoder and mask
decoder on the CPU:
encoders/sam_encoder/segment_anything/modeling/{common,transformer,mask_decoder,prompt_encoder}.py, called as predictor.py:
predict_torch calls them.  The four files need torch and numpy alone and are loaded by file under a synthetic package name (the
package's own __init__ imports torchvision, which does not exist where this runs).

The modules are filled from the recipe of tests/sam_decoder_cases.py (weights, features and prompts are pure functions of a seed:
nothing of them is recorded but the prompts).  The prompt encoder runs in float32, as the reference's does (it casts to float
itself); the decoder runs in float32 and, on the same float32 prompt tokens and positional encoding, in float64.

Per case:
  params                   h, w, B, n_points, box, multimask, input_h, input_w, seed, sharp
  coords, labels, boxes    the prompts (absent where the case has none)
  sparse                   (B, T - 5, 256) float32: the reference's sparse prompt embeddings
  ref32, ref64             the logits (B, m, 4h, 4w) - for the 64 x 64 case `sample_idx` and the logits there (the first and last
                           256 and 8192 drawn), for every edge case `sample_idx` and the logits there (all of up to 4096, else the
                           first and last 256 and 1024 drawn) - and iou32, iou64 (B, m)
  gap, gap_iou             max |ref32 - ref64| over the WHOLE output; delta = 4 gap, delta_iou = 4 gap_iou (the project's
                           convention from the SAM mask vectors)
  nopen                    the logits with |ref64| <= delta (OPEN: their sign is not decided), of the whole output
Every case but `sharp` asserts that the open logits are at most 0.1 % and takes the next seed otherwise.  `sharp` (full-scale q / k
on large features) asserts that its float64 token -> image scores exceed 88, where an exp without the running max overflows; its gap
is what it is, and the tests hold it to finiteness and its own delta only.

Run it where the reference exists (the tests read only the npz):

    python tests/golden/make_reference_sam_decoder_vectors.py [--edges-only]
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference/encoders/sam_encoder/segment_anything/modeling"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.dirname(HERE), os.path.join(ROOT, "feature-3dgs_amd")):
    sys.path.insert(0, p)
import sam_decoder_cases as cases  # noqa: E402
import sam_decoder_oracle as oracle  # noqa: E402  (the float64 scores of the sharp case only)


def load_modeling():
    pkg = types.ModuleType("ref_sam_modeling")
    pkg.__path__ = [REF]
    sys.modules["ref_sam_modeling"] = pkg
    mods = {}
    for name in ("common", "transformer", "mask_decoder", "prompt_encoder"):
        spec = importlib.util.spec_from_file_location(f"ref_sam_modeling.{name}", os.path.join(REF, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods


M = load_modeling()


def build(case, weights):
    h, w = case.grid
    pe = M["prompt_encoder"].PromptEncoder(embed_dim=256, image_embedding_size=(h, w), input_image_size=case.input_size, mask_in_chans=16)
    md = M["mask_decoder"].MaskDecoder(num_multimask_outputs=3, transformer=M["transformer"].TwoWayTransformer(depth=2, embedding_dim=256, mlp_dim=2048, num_heads=8),
                                       transformer_dim=256, iou_head_depth=3, iou_head_hidden_dim=256)
    for mod, prefix in ((pe, "prompt_encoder."), (md, "mask_decoder.")):
        sd = {k[len(prefix):]: torch.from_numpy(v) for k, v in weights.items() if k.startswith(prefix)}
        missing, unexpected = mod.load_state_dict(sd, strict=False)
        assert not unexpected and all(k.startswith("mask_downscaling.") for k in missing), (missing, unexpected)
    return pe.eval(), md.eval()


@torch.no_grad()
def record(case, seed, OUT, sample_index):
    weights = cases.make_weights(seed, case.qk_scale)
    features = torch.from_numpy(cases.make_features(case, seed))[None]
    coords, labels, boxes = cases.make_prompts(case, seed)
    pe, md = build(case, weights)
    points = None if coords is None else (torch.from_numpy(coords), torch.from_numpy(labels))
    sparse, dense = pe(points=points, boxes=None if boxes is None else torch.from_numpy(boxes), masks=None)
    assert sparse.dtype == torch.float32 and sparse.shape[1] == case.tokens - 5
    image_pe = pe.get_dense_pe()
    run = lambda dec, dt: dec(image_embeddings=features.to(dt), image_pe=image_pe.to(dt), sparse_prompt_embeddings=sparse.to(dt),
                              dense_prompt_embeddings=dense.to(dt), multimask_output=case.multimask)
    l32, i32 = run(md, torch.float32)
    l64, i64 = run(md.double(), torch.float64)
    l32, i32, l64, i64 = l32.numpy(), i32.numpy(), l64.numpy(), i64.numpy()
    h, w = case.grid
    assert l32.shape == (case.B, case.n_masks, 4 * h, 4 * w) and l32.dtype == np.float32 and l64.dtype == np.float64
    gap, gap_iou = float(np.abs(l32 - l64).max()), float(np.abs(i32 - i64).max())
    delta = 4 * gap
    nopen = int((np.abs(l64) <= delta).sum())
    if case.sharp:
        _, _, info = oracle.decode(weights, features[0], sparse, case.multimask, torch.float64)
        assert info["max_score"] > 88, info
        assert np.isfinite(l32).all() and np.isfinite(l64).all()
        print(f"{case.name}: float64 token -> image scores up to {info['max_score']:.1f}")
    elif nopen > 0.001 * l64.size:
        return False
    pre = case.name + "/"
    OUT[pre + "params"] = np.array([h, w, case.B, case.n_points, case.box, case.multimask, *case.input_size, seed, case.sharp], np.int64)
    for k, v in (("coords", coords), ("labels", labels), ("boxes", boxes)):
        if v is not None:
            OUT[pre + k] = v
    OUT[pre + "sparse"] = sparse.numpy()
    if case.sampled:
        idx = sample_index(l32.size)
        OUT[pre + "sample_idx"], OUT[pre + "ref32"], OUT[pre + "ref64"] = idx, l32.reshape(-1)[idx], l64.reshape(-1)[idx]
    else:
        OUT[pre + "ref32"], OUT[pre + "ref64"] = l32, l64
    OUT[pre + "iou32"], OUT[pre + "iou64"] = i32, i64
    OUT[pre + "gap"], OUT[pre + "gap_iou"] = np.float64(gap), np.float64(gap_iou)
    OUT[pre + "delta"], OUT[pre + "delta_iou"], OUT[pre + "nopen"] = np.float64(delta), np.float64(4 * gap_iou), np.int64(nopen)
    print(f"{case.name}: seed {seed}, logits up to {np.abs(l64).max():.3g}, gap {gap:.3g} (iou {gap_iou:.3g}), open {nopen} of {l64.size} "
          f"= {100 * nopen / l64.size:.3f} %", flush=True)
    return True


def write(file, case_list, sample_index):
    OUT = {}
    for case in case_list:
        seed = cases.SEED
        while not record(case, seed, OUT, sample_index):
            seed += 1
            assert seed < cases.SEED + 20, f"{case.name}: no seed found"
    path = os.path.join(HERE, file)
    np.savez_compressed(path, **OUT)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    assert os.path.getsize(path) < 1 << 20


def main():
    assert len(cases.CASES) == cases.N_CASES and all(c.sampled for c in cases.EDGE_CASES)
    if "--edges-only" not in sys.argv:
        write("reference_sam_decoder.npz", cases.CASES, cases.sample_index)
    write("reference_sam_decoder_edges.npz", cases.EDGE_CASES, cases.edge_sample_index)


if __name__ == "__main__":
    main()
