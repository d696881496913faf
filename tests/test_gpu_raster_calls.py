"""Characterisation of rasterization()'s host schedule.

For each kind of call that rasterization.py tells apart (which backward, harvest or not, weight store or not, which render kernel,
narrow scatter or not, alphas from the front or not), one case on the T0 scene records every Engine call the operator and its
backward make (method, engine, view, stream and a summary of the arguments) and by how much the engine's generation grew, and
compares the record with tests/golden/raster_calls.json.  The host's call order is deterministic, so this pins "same kernels, same
order, same front-cache hits" for every route through the operator.

The fixture was recorded on an MI355X with the package as it stood before the route of a view was computed in one place; regenerate
it only for an intended change of schedule:
    python tests/test_gpu_raster_calls.py --write
"""
import json
import os
import sys

import pytest
import torch

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
from test_gpu_driver_calls import Recorder, _install  # noqa: E402
from util import scene_np, to_dev  # noqa: E402

import gsbp_amd  # noqa: E402
from gsbp_amd.rasterization import get_engine, invalidate_zero_table_cache, release_engines  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raster_calls.json")
RECORDED = ["view", "project", "bin_sort", "blend_weights", "render", "render_pixels", "render_pixels_backward", "project_backward",
            "scatter", "scatter_uniform", "sh_colors", "set_narrow_scatter", "grow"]


class _Scene:
    def __init__(self, dev):
        self.cfg, sc = scene_np("T0")
        self.g = to_dev(sc, dev)
        self.dev, self.n, self.W, self.H = dev, self.cfg.n_gaussians, self.cfg.width, self.cfg.height
        self.gen = torch.Generator().manual_seed(11)
        self.gauss = tuple(self.g[k] for k in ("means", "quats", "scales", "opac"))

    def randn(self, *shape):
        return torch.randn(*shape, generator=self.gen).to(self.dev)

    def leaves(self):
        return tuple(t.clone().requires_grad_(True) for t in self.gauss)

    def call(self, colors, views=(0,), gauss=None, vms=None, **kw):
        vms = self.g["vms"][list(views)] if vms is None else vms
        Ks = self.g["K"][None].expand(len(views), 3, 3)
        return gsbp_amd.rasterization(*(gauss or self.gauss), colors, vms, Ks, self.W, self.H, **kw)

    def backward(self, out):
        """A loss whose gradient image is dense (out.sum()'s is one expanded value, a route of its own)."""
        if out.requires_grad:
            (out * self.randn(*out.shape)).sum().backward()


def _forward(d, dtype=torch.float32):
    return lambda s: s.call(s.randn(s.n, d).to(dtype))


def _harvest_passes(s):
    for d in (512, 3):  # the reference's two passes on one view: same tensor objects, the second served from the front cache
        table = torch.zeros(s.n, d, device=s.dev, requires_grad=True)
        out = s.call(table)[0]
        if d == 512:
            (out[0] * s.randn(s.H, s.W, d)).sum().backward()
        else:
            out[0].sum().backward()


def _colour_backward(s):
    s.backward(s.call(s.randn(s.n, 8).requires_grad_(True))[0])


def _geometry(d, table_grad):
    return lambda s: s.backward(s.call(s.randn(s.n, d).requires_grad_(table_grad), gauss=s.leaves())[0])


def _camera(s):
    vms = s.g["vms"][:1].clone().requires_grad_(True)
    s.backward(s.call(s.randn(s.n, 3), vms=vms, camera_grad=True)[0])


def _means2d(s):
    s.backward(s.call(s.randn(s.n, 3), views=(0, 1), means2d_grad=True)[0])


def _sh(means_grad):
    def case(s):
        gauss = (s.gauss[0].clone().requires_grad_(True),) + s.gauss[1:] if means_grad else s.gauss
        s.backward(s.call(s.randn(s.n, 4, 3), gauss=gauss, sh_degree=1)[0])
    return case


def _rgb_ed(s):
    s.backward(s.call(s.randn(s.n, 3), gauss=s.leaves(), render_mode="RGB+ED", backgrounds=s.randn(1, 4))[0])


def _two_forwards(s):
    table = s.randn(s.n, 8).requires_grad_(True)
    a, b = s.call(table, views=(0,))[0], s.call(table, views=(1,))[0]
    s.backward(a)  # the workspace holds view 1: this backward runs the front of view 0 again
    s.backward(b)


def _no_grad(s):
    with torch.no_grad():
        s.call(torch.zeros(s.n, 3, device=s.dev, requires_grad=True), gauss=s.leaves())


CASES = {
    "forward_d3": _forward(3),
    "forward_d24": _forward(24),
    "forward_bf16_d24": _forward(24, torch.bfloat16),
    "harvest_d512_then_d3": _harvest_passes,
    "colour_backward_d8": _colour_backward,
    "geometry_d3": _geometry(3, False),
    "geometry_d24_and_table": _geometry(24, True),
    "camera_grad_viewmats_only": _camera,
    "means2d_grad_two_cameras": _means2d,
    "sh1_means_grad": _sh(True),
    "sh1_no_grad": _sh(False),
    "rgb_ed_backgrounds_geometry": _rgb_ed,
    "two_forwards_then_backwards": _two_forwards,
    "no_grad_leaves_and_zero_table": _no_grad,
}


def record_all(dev):
    out = {}
    for name, case in CASES.items():
        s = _Scene(dev)
        release_engines(dev)  # every case starts on a fresh workspace: no front cache, default capacities
        invalidate_zero_table_cache()
        torch.cuda.synchronize()
        rec = Recorder()
        mp = pytest.MonkeyPatch()
        try:
            _install(mp, rec, RECORDED)
            eng = get_engine(dev, s.n, s.W, s.H)
            gen0 = eng.generation
            case(s)
            rec.calls.append(["generation", get_engine(dev, s.n, s.W, s.H).generation - gen0])
        finally:
            mp.undo()
        torch.cuda.synchronize()
        assert get_engine(dev, s.n, s.W, s.H) is eng, name
        for call in rec.calls:
            if call[0] == "sh_colors":  # (the camera centre is host float arithmetic: not part of the schedule)
                call[3].pop("campos")
        out[name] = rec.calls
    release_engines(dev)
    return json.loads(json.dumps(out))


@pytest.mark.gpu
def test_rasterization_host_calls_match_the_recorded_schedule(dev):
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
