"""Characterisation of create_feature_field's host schedule.

For one small T1 job per schedule, the test records every Engine call the driver makes (method, engine, view, stream and a
summary of the arguments), every feature_fn call and the ViewPipeline constructor arguments, and compares the record with
tests/golden/driver_calls.json.  The host's call order is deterministic, so this pins "same kernels, same order, same
feature_fn calls" for every schedule of the driver.

The fixture was recorded on an MI355X; regenerate it only for an intended change of schedule:
    python tests/test_gpu_driver_calls.py --write
"""
import inspect
import json
import os
import sys

import pytest
import torch

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
from util import scene_np, to_dev  # noqa: E402

import gsbp_amd  # noqa: E402
from gsbp_amd import backproject as bp  # noqa: E402
from gsbp_amd import synthetic as syn  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "driver_calls.json")
N_VIEWS = 4

# Engine methods that launch work or change an engine's state (the predicates can_* are pure and not recorded)
RECORDED = ["view", "project", "bin_sort", "blend_weights", "blend_scatter", "blend_scatter_encoded", "blend_tokens",
            "scatter_tokens", "scatter", "scatter_encoded", "backproject_view", "encode_map", "accumulate_stats", "grow",
            "finalize", "set_narrow_scatter", "set_front_priority", "set_split_encoder", "bind_stream"]


class Recorder:
    def __init__(self):
        self.calls = []
        self.ids = {}  # (kind, key) -> ordinal in order of first appearance
        self.alive = []  # the engines seen: an engine freed during the job must not hand its id() to a later one

    def ordinal(self, kind, key):
        return self.ids.setdefault((kind, key), sum(1 for k in self.ids if k[0] == kind))

    def engine(self, e):
        if ("engine", id(e)) not in self.ids:
            self.alive.append(e)
        return self.ordinal("engine", id(e))

    def summary(self, x):
        if isinstance(x, torch.Tensor):
            return ["tensor", list(x.shape), str(x.dtype)]
        if isinstance(x, gsbp_amd.Engine):
            return ["engine", self.engine(x)]
        if isinstance(x, gsbp_amd._lib.View):
            return ["view", getattr(x, "_rec_id", None)]
        if isinstance(x, torch.cuda.Stream):
            return ["stream", self.ordinal("stream", x.cuda_stream)]
        if isinstance(x, float):
            return round(x, 9)
        if isinstance(x, (list, tuple)):
            return [self.summary(y) for y in x]
        if isinstance(x, dict):
            return {k: self.summary(v) for k, v in sorted(x.items())}
        if x is None or isinstance(x, (bool, int, str)):
            return x
        return type(x).__name__

    def bound(self, fn, args, kw):
        b = inspect.signature(fn).bind(*args, **kw)
        b.apply_defaults()
        return {k: self.summary(v) for k, v in b.arguments.items() if k not in ("self", "viewmat", "K")}


def _install(monkeypatch, rec, names=RECORDED):
    E = gsbp_amd.Engine

    def wrap(name, orig):
        def f(self, *a, **k):
            args = rec.bound(orig, (self,) + a, k)
            stream = rec.ordinal("stream", self._stream().value or 0)
            rec.calls.append([name, rec.engine(self), stream, args])
            out = orig(self, *a, **k)
            if name == "view":
                out._rec_id = sum(1 for c in rec.calls if c[0] == "view") - 1
            return out
        return f

    for name in names:
        monkeypatch.setattr(E, name, wrap(name, getattr(E, name)))
    orig_init = E.__init__

    def init(self, *a, **k):
        orig_init(self, *a, **k)
        rec.calls.append(["Engine", rec.engine(self), rec.bound(orig_init, (self,) + a, k)])
    monkeypatch.setattr(E, "__init__", init)
    orig_pipe = bp.ViewPipeline.__init__

    def pipe_init(self, *a, **k):
        rec.calls.append(["ViewPipeline", rec.bound(orig_pipe, (self,) + a, k)])
        orig_pipe(self, *a, **k)
    monkeypatch.setattr(bp.ViewPipeline, "__init__", pipe_init)


def _cases():
    """name -> (keyword arguments of create_feature_field, map kind).  Map kinds: ("full", D), ("low", h, w, D), ("enc", K, n)."""
    return {
        "d24_pipelined": (dict(), ("full", 24)),
        "d24_serial": (dict(pipeline=False), ("full", 24)),
        "d24_depth2": (dict(pipeline=2), ("full", 24)),
        "d256_wide_pipelined": (dict(), ("full", 256)),
        "d256_wide_serial": (dict(pipeline=False), ("full", 256)),
        "d24_no_fuse_small": (dict(fuse_small=False), ("full", 24)),
        "d24_no_fuse_small_serial": (dict(fuse_small=False, pipeline=False), ("full", 24)),
        "encoder_in_blend_split": (dict(encoder_split=True), ("enc", 64, 16)),
        "encoder_in_blend_nosplit": (dict(encoder_split=False), ("enc", 64, 16)),
        "encoder_fused_staging": (dict(fuse_encoder=True), ("enc", 64, 16)),
        "encoder_ahead": (dict(encoder_in_blend=False), ("enc", 64, 16)),
        "encoder_serial": (dict(pipeline=False), ("enc", 64, 16)),
        "nearest_tokens": (dict(upsample="nearest", reduction="mean"), ("low", 8, 12, 256)),
        "nearest_tokens_serial": (dict(upsample="nearest", reduction="mean", pipeline=False), ("low", 8, 12, 256)),
        "nearest_no_tokens": (dict(upsample="nearest", reduction="mean", token_space=False), ("low", 8, 12, 256)),
        "nearest_stream_safe": (dict(upsample="nearest", token_space=False, feature_fn_stream_safe=True), ("low", 12, 17, 24)),
        "bilinear": (dict(upsample="bilinear"), ("low", 12, 17, 128)),
        "bilinear_serial": (dict(upsample="bilinear", pipeline=False), ("low", 12, 17, 128)),
        "fisheye_serial_d24": (dict(pipeline=False, camera_model="fisheye"), ("full", 24)),
        "fisheye_serial_d256": (dict(pipeline=False, camera_model="fisheye", rasterize_mode="antialiased"), ("full", 256)),
        "grow_pipelined": (dict(engine="small"), ("full", 24)),
        "grow_serial": (dict(engine="small", pipeline=False), ("full", 24)),
    }


def record_all(dev):
    from _pytest.monkeypatch import MonkeyPatch
    cfg, sc = scene_np("T1", n_views=N_VIEWS)
    g = to_dev(sc, dev)
    vms = syn.make_cameras(cfg, n_views=N_VIEWS).to(dev)
    bp.wide_kernel_selfcheck(dev)  # once per process: keep its own Engine calls out of the records
    out = {}
    for name, (kw, kind) in _cases().items():
        gen = torch.Generator().manual_seed(7)
        if kind[0] == "full":
            maps, dim = [torch.randn(cfg.height, cfg.width, kind[1], generator=gen) for _ in range(N_VIEWS)], kind[1]
        elif kind[0] == "low":
            maps, dim = [torch.randn(kind[1], kind[2], kind[3], generator=gen) for _ in range(N_VIEWS)], kind[3]
        else:
            maps, dim = [torch.randn(cfg.height, cfg.width, kind[1], generator=gen) for _ in range(N_VIEWS)], kind[1]
            kw = dict(kw, encoder=(torch.randn(kind[1], kind[2], generator=gen) / kind[1] ** 0.5).to(dev))
        maps = [m.to(dev) for m in maps]
        if kw.get("engine") == "small":
            kw = dict(kw, engine=gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev, isect_cap=3000,
                                                 pair_cap=1 << 15, tight_binning=True))
        torch.cuda.synchronize()
        rec = Recorder()
        mp = MonkeyPatch()
        try:
            _install(mp, rec)

            def feature_fn(v):
                rec.calls.append(["feature_fn", v])
                return maps[v]
            _, _, _, st = gsbp_amd.create_feature_field(g["means"], g["quats"], g["scales"], g["opac"], vms, g["K"],
                                                        cfg.width, cfg.height, feature_fn, dim, return_partials=True, **kw)
        finally:
            mp.undo()
        torch.cuda.synchronize()
        assert st["overflow"] == 0, name
        out[name] = rec.calls
    return json.loads(json.dumps(out))


@pytest.mark.gpu
def test_driver_host_calls_match_the_recorded_schedule(dev):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = record_all(dev)
    assert sorted(got) == sorted(want)
    for name in want:
        first = next((i for i, (a, b) in enumerate(zip(got[name], want[name])) if a != b), min(len(got[name]), len(want[name])))
        assert got[name] == want[name], (name, first, got[name][first:first + 1], want[name][first:first + 1])


if __name__ == "__main__":
    if "--write" in sys.argv:
        path = sys.argv[sys.argv.index("--write") + 1] if len(sys.argv) > sys.argv.index("--write") + 1 else GOLDEN
        rec = record_all(torch.device("cuda:0"))
        with open(path, "w") as f:
            json.dump(rec, f, indent=0, separators=(",", ":"))
            f.write("\n")
        print("wrote", path, {k: len(v) for k, v in rec.items()})
