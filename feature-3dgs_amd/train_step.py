"""Data-parallel training step around the drop-in op.

One call = the body of the reference's training loop between "pick a camera" and "optimizer step"
(reference train.py:84-149): render, loss, backward, densification statistics.  With one process (world size 1)
and one view per step it performs exactly the reference's updates:

    train.py:91        render_pkg = render(viewpoint_cam, gaussians, pipe, background)
    train.py:98-106    loss = (1-l) L1 + l (1 - ssim) + L1_feature        -> `loss_fn(render_pkg, camera)`
    train.py:108       loss.backward()
    train.py:132       gaussians.max_radii2D[vis] = max(gaussians.max_radii2D[vis], radii[vis])
    train.py:133       gaussians.add_densification_stats(viewspace_point_tensor, vis)
                       (scene/gaussian_model.py:436-438: xyz_gradient_accum[vis] += |grad_xy|, denom[vis] += 1)

With N processes (one per GPU, `torch.distributed` initialised) every rank renders ITS views of the same Gaussians;
afterwards every rank holds, for every parameter, the SUM of the gradients over all ranks' views (`dp.dp_step`), and
the densification statistics of all views (per-step deltas reduced with SUM / SUM / MAX), so the replicas stay
identical whatever they do next (optimizer step, densify_and_prune).  N views per step instead of one is a change of
the training recipe ABOVE the op - the op, its gradients and the statistics per view are the reference's.

`model` is duck-typed like the reference's `GaussianModel`: it needs `max_radii2D`, `xyz_gradient_accum`, `denom`
(tensors of length P) and the parameter tensors named in `param_names` (default: the reference's `_xyz`,
`_features_dc`, `_features_rest`, `_opacity`, `_scaling`, `_rotation`, `_semantic_feature`, scene/gaussian_model.py:41-50).
"""
from __future__ import annotations

from typing import Callable, Dict, Iterable, NamedTuple, Optional, Sequence

import torch

import dp

REFERENCE_PARAM_NAMES = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation", "_semantic_feature")


class StepResult(NamedTuple):
    loss: torch.Tensor                    # sum over this rank's views (detached)
    views: int                            # views rendered by this rank
    grads: Dict[str, torch.Tensor]        # name -> summed gradient (the tensors in `param.grad`)


def densification_deltas(render_pkg: dict, P: int, device) -> tuple:
    """The per-view increments of scene/gaussian_model.py:436-438 and train.py:132, as dense tensors."""
    vis = render_pkg["visibility_filter"]
    vsp = render_pkg["viewspace_points"]
    g = vsp.grad if vsp.grad is not None else torch.zeros_like(vsp)
    norm = torch.zeros(P, 1, device=device)
    norm[vis] = torch.norm(g[vis, :2], dim=-1, keepdim=True)
    count = torch.zeros(P, 1, device=device)
    count[vis] = 1.0
    radii = torch.zeros(P, device=device, dtype=torch.float32)
    radii[vis] = render_pkg["radii"][vis].float()
    return norm, count, radii


def dp_train_step(render: Callable, loss_fn: Callable, model, cameras: Iterable, pipe, background: torch.Tensor,
                  group=None, overlap: bool = True, param_names: Sequence[str] = REFERENCE_PARAM_NAMES,
                  feature_param: str = "_semantic_feature", densification_stats: bool = True,
                  sh_params: Sequence[str] = ("_features_dc", "_features_rest"), rows_chunks: int = 4,
                  reduce: bool = True, fused_stats: bool = False) -> StepResult:
    """Render + loss + backward for this rank's `cameras`, then make gradients and densification statistics
    global.  `render(camera, model, pipe, background)` is the reference's `gaussian_renderer.render`;
    `loss_fn(render_pkg, camera)` returns the scalar loss of one view.  The optimizer step stays with the caller
    (train.py:146-151), exactly as in the reference.  `sh_params`: the parameters that receive nothing but the op's SH
    gradient (scene/gaussian_model.py:113-116: get_features = cat(_features_dc, _features_rest)); with `overlap` their
    all-reduce runs in `rows_chunks` row ranges inside the backward pass (empty: reduce them afterwards).
    `reduce=False`: the gradients stay LOCAL to the rank (the densification statistics are still made global) - for a sharded
    optimizer, whose reduce-scatter is the exchange: `dp.ShardedOptimizer(...).step(result.grads)` (half the gradient
    bytes of the all-reduce, optimizer work and state divided by the world size).
    `fused_stats`: the densification statistics through `model_front.densification_stats` (one launch per view on zeroed
    buffers for the deltas, one more for the model's radii) instead of boolean-mask indexing: nothing is read back to the host."""
    params = {n: getattr(model, n) for n in param_names if getattr(model, n, None) is not None}
    cameras = list(cameras)
    P = next(iter(params.values())).shape[0]
    device = next(iter(params.values())).device
    pkgs, losses = [], []

    def render_and_backward(i):
        pkg = render(cameras[i], model, pipe, background)
        loss = loss_fn(pkg, cameras[i])
        loss.backward()
        pkgs.append(pkg)
        losses.append(loss.detach())

    def forward(i):
        pkg = render(cameras[i], model, pipe, background)
        loss = loss_fn(pkg, cameras[i])
        pkgs.append(pkg)
        losses.append(loss.detach())
        return loss

    # the overlap needs the feature parameter to be the op's direct input (true for the reference's model:
    # get_semantic_feature returns the parameter itself, scene/gaussian_model.py:121-123)
    if len(cameras) > 1:
        # several views per rank: pipelined over two streams, the feature gradient accumulated in place across the views and
        # reduced from inside the last view's backward pass (dp.dp_step_views)
        grads = dp.dp_step_views(forward, lambda loss: loss.backward(), params, range(len(cameras)), group=group,
                                 overlap=overlap and reduce, feature_key=feature_param,
                                 accumulate=None if overlap else False, reduce=reduce)
    else:
        grads = dp.dp_step(render_and_backward, params, range(len(cameras)), group=group,
                           overlap=overlap and reduce and len(cameras) == 1, feature_key=feature_param,
                           rows_leaves={"sh": tuple(sh_params)} if sh_params else None, rows_chunks=rows_chunks, reduce=reduce)

    if densification_stats and fused_stats:
        import model_front
        with torch.no_grad():
            norm = torch.zeros(P, 1, device=device)
            count = torch.zeros(P, 1, device=device)
            radii = torch.zeros(P, device=device, dtype=torch.float32)
            for pkg in pkgs:        # the deltas of all views: the kernel adds into the zeroed buffers
                model_front.densification_stats(pkg["viewspace_points"].grad, pkg["radii"], norm, count, radii)
            dp.reduce_densification_stats(norm, count, radii, group=group)
            model.xyz_gradient_accum += norm
            model.denom += count
            # the second call: max_radii2D = max(max_radii2D, radii) where a view saw the Gaussian (radii > 0), else untouched
            model_front.densification_stats(None, radii.to(torch.int32), None, None, model.max_radii2D)
    elif densification_stats:
        with torch.no_grad():
            norm = torch.zeros(P, 1, device=device)
            count = torch.zeros(P, 1, device=device)
            radii = torch.zeros(P, device=device, dtype=torch.float32)
            for pkg in pkgs:
                n, c, r = densification_deltas(pkg, P, device)
                norm += n
                count += c
                radii = torch.maximum(radii, r)
            dp.reduce_densification_stats(norm, count, radii, group=group)
            model.xyz_gradient_accum += norm
            model.denom += count
            seen = count.squeeze(-1) > 0
            mr = model.max_radii2D
            mr[seen] = torch.maximum(mr[seen], radii[seen].to(mr.dtype))
    total = torch.stack(losses).sum() if losses else torch.zeros((), device=device)
    return StepResult(total, len(cameras), grads)


def _default_set_band(r0: int, r1: int) -> None:
    from diff_gaussian_rasterization import _C
    _C.set_tile_band(r0, r1)


def dp_train_step_bands(render: Callable, loss_fn: Callable, model, camera, pipe, background: torch.Tensor, group=None,
                        param_names: Sequence[str] = REFERENCE_PARAM_NAMES, densification_stats: bool = True,
                        image_keys: Sequence[str] = ("render", "feature_map", "depth"), reduce: bool = True,
                        set_band: Callable[[int, int], None] = _default_set_band) -> StepResult:
    """ONE view split over the ranks by tile rows ("alternative for single huge views"; include/f3dgs.h:
    f3dgs_set_tile_band) - for steps that have fewer views than GPUs.  Every rank renders the same `camera` restricted to its
    band of 16-pixel tile rows (`dp.band_rows`), the bands are gathered into whole images (`dp.gather_bands` on
    `render_pkg[k]` for k in `image_keys`: the images the loss reads), `loss_fn(render_pkg, camera)` sees the whole view on
    every rank - so window-based terms such as SSIM are exact at the band borders - and its backward pass reaches this rank's
    rows only; the gradients of the ranks then SUM to the whole view's gradient (`dp.all_reduce_gaussian_grads`), the radii MAX
    to the whole view's, and the densification statistics are those of ONE view: |sum of the screen-space gradients| and one
    visibility count per Gaussian seen in any band (scene/gaussian_model.py:436-438).  The loss returned is the whole view's, the
    same on every rank."""
    params = {n: getattr(model, n) for n in param_names if getattr(model, n, None) is not None}
    P = next(iter(params.values())).shape[0]
    device = next(iter(params.values())).device
    world = torch.distributed.get_world_size(group) if dp._active(group) else 1
    rank = torch.distributed.get_rank(group) if world > 1 else 0
    H = int(camera.image_height)
    r0, r1, _y0, _y1 = dp.band_rows(H, rank, world)
    for p in params.values():
        p.grad = None
    if world > 1:       # (1 << 20: "an empty band", the share of a rank beyond the last tile row)
        set_band(r0, r1) if r1 > r0 else set_band(1 << 20, 1 << 20)
    try:
        pkg = render(camera, model, pipe, background)
    finally:
        if world > 1:
            set_band(0, 0)
    whole = dict(pkg)
    for k in image_keys:
        if k in whole and isinstance(whole[k], torch.Tensor) and whole[k].dim() >= 2 and whole[k].numel():
            whole[k] = dp.gather_bands(whole[k], group=group)
    loss = loss_fn(whole, camera)
    loss.backward()
    grads = {n: (p.grad if p.grad is not None else torch.zeros_like(p)) for n, p in params.items()}
    for n, p in params.items():
        p.grad = grads[n]
    if reduce and world > 1:
        dp.all_reduce_gaussian_grads(grads, group=group)
    if densification_stats:
        with torch.no_grad():
            vsp = pkg["viewspace_points"]
            g2 = (vsp.grad if vsp.grad is not None else torch.zeros_like(vsp))[:, :2].contiguous()
            radii = pkg["radii"].float().clone()
            if world > 1:       # one view: its screen-space gradient is the SUM over the bands, its radii their MAX
                torch.distributed.all_reduce(g2, op=torch.distributed.ReduceOp.SUM, group=group)
                torch.distributed.all_reduce(radii, op=torch.distributed.ReduceOp.MAX, group=group)
            seen = radii > 0
            norm = torch.zeros(P, 1, device=device)
            norm[seen] = torch.norm(g2[seen], dim=-1, keepdim=True)
            model.xyz_gradient_accum += norm
            model.denom += seen.float().unsqueeze(-1)
            mr = model.max_radii2D
            mr[seen] = torch.maximum(mr[seen], radii[seen].to(mr.dtype))
    return StepResult(loss.detach(), 1, grads)


class CapturedTrainer:
    """One WHOLE training iteration replayed from a HIP graph: the body of train.py:77-149 with nothing returning
    to the host -

        zero_grad(set_to_none=True); render; loss_fn(render_pkg, *targets); backward; add_densification_stats;
        model.optimizer.step(); the decoder's optimizer, if one was given

    `model.optimizer` must be a `FusedAdam(capturable=True)`: its step counts, rates and schedule live on the device, so a
    replay takes the step it runs in.  `step(camera, *targets)` returns the detached loss and `radii` (static tensors of the
    graph: valid until the next `step`); `render_pkg` and every parameter's `.grad` are those of the last replay.

    Graphs are built with `graph_step.CapturedStep` and cached by everything a capture freezes: image size, FoVx / FoVy,
    `active_sh_degree`, the addresses and row count of the model's parameters and statistics, the background's address, the targets' shapes
    and the optimizer's `schedule_epoch`.  View matrices, camera centre and targets are copied into static tensors before a
    replay, so cameras that differ only in pose share one graph.  A changed key captures again (least recently used graph
    evicted at `max_graphs`): `densify` needs no notification - it moves the parameters, and that changes the key;
    `model_front.reset_opacity_` keeps the addresses and so the graph.  The warm-up iterations a capture needs are undone:
    parameters, optimizer state and densification statistics are saved before them and written back in place.

    `check()` (it synchronises) is `CapturedStep.check()` for the graph last replayed: False says that the frames since the
    last check did not fit the instance provision - their iterations stepped on incomplete gradients - and that the graph was
    captured again with room.  `loss_fn` and `render` may call the rasterizer once per iteration (CapturedStep's rule)."""

    def __init__(self, model, loss_fn: Callable, pipe, background: torch.Tensor, render: Optional[Callable] = None,
                 max_graphs: int = 4, visibility: bool = False, decoder_optimizer=None,
                 param_names: Sequence[str] = REFERENCE_PARAM_NAMES):
        import model_front
        opt = getattr(model, "optimizer", None)
        if opt is None or not getattr(opt, "capturable", False):
            raise TypeError("CapturedTrainer: model.optimizer must be a FusedAdam(capturable=True) - a host-side step count "
                            "would be frozen into the graph")
        self.model, self.loss_fn, self.pipe, self.background = model, loss_fn, pipe, background
        self.render = render if render is not None else model_front.render
        self.max_graphs = max(1, int(max_graphs))
        self.visibility = bool(visibility)
        self.decoder_optimizer = decoder_optimizer
        self.param_names = tuple(param_names)
        self.captures = 0
        self.render_pkg = None
        self._graphs = {}          # key -> entry, in order of last use (dicts keep insertion order)
        self._stream = None        # one capture stream for every graph: the parameters' gradient accumulators stay on it
        self._current = None

    # -- what a capture freezes ---------------------------------------------------------------------------------------------------
    def _params(self):
        return {n: getattr(self.model, n) for n in self.param_names if getattr(self.model, n, None) is not None}

    def _key(self, camera, targets):
        params = self._params()
        return (int(camera.image_height), int(camera.image_width), float(camera.FoVx), float(camera.FoVy),
                int(self.model.active_sh_degree), tuple((n, p.data_ptr(), tuple(p.shape)) for n, p in params.items()),
                tuple(getattr(self.model, n).data_ptr() for n in ("xyz_gradient_accum", "denom", "max_radii2D")),
                self.background.data_ptr(), tuple((tuple(t.shape), t.dtype) for t in targets),
                self.model.optimizer.schedule_epoch)

    # -- state the warm-up iterations of a capture must not leave changed --------------------------------------------------------
    def _mutable_state(self):
        out = [p.detach() for p in self._params().values()]
        out += self.model.optimizer.device_state()
        out += [getattr(self.model, n) for n in ("xyz_gradient_accum", "denom", "max_radii2D")]
        dec = self.decoder_optimizer
        if dec is not None:
            for g in dec.param_groups:
                out += [p.detach() for p in g["params"]]
            for st in dec.state.values():
                out += [v for v in st.values() if torch.is_tensor(v)]
        return [t for t in out if t.numel()]

    @staticmethod
    def _slot(t):
        return (t.data_ptr(), t.numel(), t.dtype)

    def _capture_keeping_state(self, capture):
        saved = {self._slot(t): t.clone() for t in self._mutable_state()}
        try:
            return capture()
        finally:
            with torch.no_grad():
                for t in self._mutable_state():       # state the warm-up created (a first ever step) goes back to zeros
                    old = saved.get(self._slot(t))
                    t.copy_(old) if old is not None else t.zero_()
            self.captures += 1

    def _build(self, camera, targets):
        import types
        import model_front
        from graph_step import CapturedStep
        cam = types.SimpleNamespace(image_height=int(camera.image_height), image_width=int(camera.image_width),
                                    FoVx=float(camera.FoVx), FoVy=float(camera.FoVy),
                                    world_view_transform=camera.world_view_transform.detach().clone(),
                                    full_proj_transform=camera.full_proj_transform.detach().clone(),
                                    camera_center=camera.camera_center.detach().clone())
        static_targets = [t.detach().clone() for t in targets]
        model, opt, dec = self.model, self.model.optimizer, self.decoder_optimizer
        held = {}

        def iteration():
            opt.zero_grad(set_to_none=True)
            if dec is not None:
                dec.zero_grad(set_to_none=True)
            pkg = self.render(cam, model, self.pipe, self.background)
            loss = self.loss_fn(pkg, *static_targets)
            loss.backward()
            model_front.add_densification_stats(model, pkg)
            opt.step(visibility=pkg["radii"] if self.visibility else None)
            if dec is not None:
                dec.step()
            held["grads"] = {n: p.grad for n, p in self._params().items()}
            return loss.detach(), pkg

        if self._stream is None:
            self._stream = torch.cuda.Stream()
        step = CapturedStep(iteration, stream=self._stream)
        self._capture_keeping_state(step.capture)
        return types.SimpleNamespace(step=step, camera=cam, targets=static_targets, held=held)

    def step(self, camera, *targets):
        key = self._key(camera, targets)
        entry = self._graphs.pop(key, None)
        if entry is None:
            entry = self._build(camera, targets)
            while len(self._graphs) >= self.max_graphs:
                self._graphs.pop(next(iter(self._graphs)))
        self._graphs[key] = entry
        self._current = entry
        # pose and targets into the graph's static tensors: ONE multi-tensor copy launch; a target that already IS the static
        # tensor (`static_targets`: a data loader may write there directly) costs nothing
        pairs = [(getattr(entry.camera, n), getattr(camera, n)) for n in ("world_view_transform", "full_proj_transform", "camera_center")]
        pairs += [(d, s) for d, s in zip(entry.targets, targets) if d.data_ptr() != s.data_ptr()]
        with torch.no_grad():
            if all(d.dtype == s.dtype and d.device == s.device and d.shape == s.shape for d, s in pairs):
                torch._foreach_copy_([d for d, _ in pairs], [s for _, s in pairs])
            else:
                for d, s in pairs:
                    d.copy_(s)
        loss, pkg = entry.step.replay()
        params = self._params()
        for n, g in entry.held["grads"].items():        # the gradients this graph writes (another graph's may be attached)
            params[n].grad = g
        self.render_pkg = pkg
        return loss, pkg["radii"]

    @property
    def static_targets(self):
        """The target tensors the graph last replayed reads: `step` skips the copy of a target that is one of these."""
        return None if self._current is None else list(self._current.targets)

    def check(self) -> bool:
        if self._current is None:
            return True
        c = self._current.step.counts()
        if c is None or (c[4] == 0 and c[0] <= c[3]):
            return True
        return self._capture_keeping_state(self._current.step.check)
