"""Generates tests/golden/reference_lpips.npz by running the reference's own lpipsPyTorch on the CPU: modules/{utils,networks,
lpips}.py - BaseNet.forward, LinLayers, normalize_activation, LPIPS.forward - in float32 and in float64, loaded by file under a
synthetic package name.  `torchvision.models` is a stub in sys.modules whose vgg16 returns an nn.Sequential with torchvision's
`features` layout, filled from the case; nothing may reach the network: before anything is constructed `get_state_dict` in the
loaded module returns the case's heads and torch.hub.load_state_dict_from_url raises.

Weights, images and pairs are the recipe of tests/lpips_cases.py (pure functions of a seed: none of them is recorded).

Per case:
  params                H, W, N, seed, dead, samples
  tap64_{l}             the float64 tap l of all 2N images (x first, then y), flattened, at cases.sample_index(size, samples, l)
                        (the whole tensor where it is smaller: a committed file holds 1 MB, the taps of one case alone several)
  gap_tap               (5,) max |tap32 - tap64| over the WHOLE tensor of each layer
  terms32 / terms64     (N, 5) layer terms, total32 / total64 (N,), dropin32 / dropin64 the (1,1,1,1) value of LPIPS.forward
  gap_rel               max over cases.GAP_SEEDS seeds, pairs and layers of |d32 - d64| / d64, pairs with `y is x` and terms that
                        are 0 left out (a scalar's gap can be small by luck at one seed); only the first seed is recorded
`names` / `shapes`: the reference's LPIPS.state_dict() keys.  The bars of the tests are 4 x these gaps.  Asserted here: the
reference's float32 meets the bars with a factor of 1, and `dead`'s fifth term is exactly 0 in both precisions.

Run it where the reference exists (the tests read only the npz):

    python tests/golden/make_reference_lpips_vectors.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

REF = "/root/reference/lpipsPyTorch/modules"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import lpips_cases as cases  # noqa: E402

CURRENT = {}          # the weights the stubs hand out


def _vgg16(*args, **kwargs):
    layers, cin = [], 3
    for v in (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"):      # torchvision's cfg "D"
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    net = types.SimpleNamespace(features=nn.Sequential(*layers))
    sd = {k[len("features."):]: torch.from_numpy(v) for k, v in CURRENT["weights"].items() if k.startswith("features.")}
    net.features.load_state_dict(sd, strict=True)
    return net


def load_reference():
    def refuse(*a, **k):
        raise RuntimeError("the golden generator must not reach the network")
    torch.hub.load_state_dict_from_url = refuse
    tv = types.ModuleType("torchvision")
    tv.models = types.ModuleType("torchvision.models")
    tv.models.vgg16 = _vgg16
    tv.models.VGG16_Weights = types.SimpleNamespace(IMAGENET1K_V1=None)
    sys.modules["torchvision"], sys.modules["torchvision.models"] = tv, tv.models
    pkg = types.ModuleType("ref_lpips_modules")
    pkg.__path__ = [REF]
    sys.modules["ref_lpips_modules"] = pkg
    mods = {}
    for name in ("utils", "networks", "lpips"):
        spec = importlib.util.spec_from_file_location(f"ref_lpips_modules.{name}", os.path.join(REF, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    # the heads under the reference's renamed keys, as its get_state_dict returns them
    mods["lpips"].get_state_dict = lambda net_type, version: {f"{i}.1.weight": torch.from_numpy(CURRENT["weights"][f"lin.{i}.weight"]) for i in range(5)}
    return mods


M = load_reference()
OUT = {}


@torch.no_grad()
def run(model, x, y, dtype):
    """(raw taps of cat(x, y), (N,5) terms, (N,) totals, (1,1,1,1) drop-in value) of the reference's modules in dtype"""
    model = model.to(dtype)
    x, y = torch.from_numpy(x).to(dtype), torch.from_numpy(y).to(dtype)
    keep = M["networks"].normalize_activation
    M["networks"].normalize_activation = lambda t, eps=1e-10: t          # BaseNet.forward without the normalisation: the raw taps
    raw = model.net(torch.cat([x, y]))
    M["networks"].normalize_activation = keep
    feat_x, feat_y = model.net(x), model.net(y)
    res = [lin((fx - fy) ** 2).mean((2, 3), True) for fx, fy, lin in zip(feat_x, feat_y, model.lin)]
    terms = torch.cat(res, 1)[:, :, 0, 0]
    total = torch.sum(torch.cat([r[None] for r in res], 0), 0)[:, 0, 0, 0]
    return raw, terms.numpy(), total.numpy(), model(x, y).numpy()


def record(case):
    gap_rel = 0.0
    for s in range(cases.GAP_SEEDS):
        seed = cases.SEED + s
        CURRENT["weights"] = cases.make_weights(seed, case.dead)
        model = M["lpips"].LPIPS("vgg", "0.1").eval()
        x, y = cases.make_pairs(case, seed)
        raw32, t32, tot32, drop32 = run(model, x, y, torch.float32)
        raw64, t64, tot64, drop64 = run(model, x, y, torch.float64)
        live = np.array([k != "same" for k in case.kinds])[:, None] & (t64 > 0)
        rel = np.abs(t32 - t64)[live] / t64[live]
        rel_tot = np.abs(tot32 - tot64)[live.any(1)] / tot64[live.any(1)]
        gap_rel = max(gap_rel, float(rel.max()), float(rel_tot.max()))
        if s:
            continue
        pre = case.name + "/"
        if not OUT:
            sd = model.state_dict()
            OUT["names"] = np.array(list(sd.keys()))
            OUT["shapes"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
        OUT[pre + "params"] = np.array([case.H, case.W, len(case.kinds), seed, case.dead, case.samples], np.int64)
        gap_tap = []
        for l, (a, b) in enumerate(zip(raw32, raw64)):
            assert tuple(b.shape) == cases.tap_shapes(case)[l] and a.dtype == torch.float32 and b.dtype == torch.float64
            gap_tap.append(float((a.double() - b).abs().max()))
            OUT[pre + f"tap64_{l}"] = b.reshape(-1).numpy()[cases.sample_index(b.numel(), case.samples, l)]
        OUT[pre + "gap_tap"] = np.array(gap_tap)
        OUT[pre + "terms32"], OUT[pre + "terms64"], OUT[pre + "total32"], OUT[pre + "total64"] = t32, t64, tot32, tot64
        OUT[pre + "dropin32"], OUT[pre + "dropin64"] = drop32, drop64
        assert drop64.shape == (1, 1, 1, 1) and abs(drop64.item() - tot64.sum()) <= 1e-12 * max(1.0, abs(drop64.item()))
        if case.dead:
            assert (t32[:, 4] == 0).all() and (t64[:, 4] == 0).all() and all(float(r[4].abs().max()) == 0 for r in (raw32, raw64))
        for k, kind in enumerate(case.kinds):
            if kind == "same":
                assert (t32[k] == 0).all() and (t64[k] == 0).all()
        first = (t32, t64, tot32, tot64)
    t32, t64, tot32, tot64 = first
    OUT[case.name + "/gap_rel"] = np.float64(gap_rel)
    assert (np.abs(t32 - t64) <= gap_rel * t64).all() and (np.abs(tot32 - tot64) <= gap_rel * tot64).all()      # factor 1
    print(f"{case.name}: totals {tot64}, gap_tap {np.array2string(OUT[case.name + '/gap_tap'], precision=3)}, gap_rel {gap_rel:.3g}", flush=True)


def main():
    for case in cases.CASES:
        record(case)
    path = os.path.join(HERE, "reference_lpips.npz")
    np.savez_compressed(path, **OUT)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
