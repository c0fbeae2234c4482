"""One layout object behind both front doors, without a GPU: `MPI.render_views_shared` / `render_views_depth` and `MPIRenderer.render_shared` /
`render_depth` build their launch through the same two constructors (`hip_mpi._shared_layout`, `_depth_layout`), so the same inputs must reach the
C ABI as the same entries with the same structs, forward and backward, whichever door they came through (test_marshal_cpu's recorder); and the
five keywords the layout object replaced are refused by name."""
import os
import warnings

import pytest
import torch

from test_depth_alpha_cpu import depth_inputs, rec  # noqa: F401  (rec: the recorder fixture rec2 builds on)
from test_depth_alpha_window_cpu import rec2  # noqa: F401  (the recorder that knows every entry of both layouts and answers the window query)
from test_marshal_cpu import SAME_POINTERS, D, H, M, W, loss_of, make_inputs, scalars_of, shared_inputs

SHARED = ("gmpi_mpi_render_shared_launch", "gmpi_mpi_render_shared_backward_launch")
DEPTH_BACKWARD = {"pixel": "gmpi_mpi_render_depth_backward_launch", "tile": "gmpi_mpi_render_depth_backward_tile_launch"}
REMOVED_KEYWORDS = ("_shared", "_shared_variant", "_depth", "_depth_backward", "_depth_forward")


def renderer_and_cameras(geo):
    """A renderer of D planes at the marshalling shape (set_cam takes squares only: the size is set by hand, no ray is made here) and the
    views of `geo` as `given_cam_infos`; its own plane geometry for M MPIs, which is what both doors are given."""
    from ml_gmpi_amd import make_renderer
    _, ray, eye, zd = geo
    r = make_renderer("FFHQ", n_planes=D, device=torch.device("cpu"), ray_backend="torch")
    r.render_h, r.render_w = H, W
    infos = dict(batch_yaws=torch.zeros((M, 1)), batch_pitches=torch.zeros((M, 1)), batch_tf_c2w=torch.eye(4).repeat(M, 1, 1),
                 batch_ray_dir=ray, batch_eye_pos=eye, batch_z_dir=zd)
    return r, infos, r._dhw_for(M)


def both_doors(rec, through_mpi, through_renderer, inputs, uses_T):
    """Forward and backward through either door, on the same tensors; returns the two call lists."""
    runs = []
    for door in (through_mpi, through_renderer):
        del rec.calls[:]
        for t in inputs:
            if t is not None:
                t.requires_grad_(True).grad = None
        color, depth, T = door()
        loss_of(dict(color=color, depth=depth, T=T), uses_T).backward()
        assert all(t is None or (t.grad is not None and t.grad.shape == t.shape) for t in inputs)
        runs.append(list(rec.calls))
    return runs


def assert_same_calls(a, b, n_structs):
    """The same entries in the same order (which ones: test_renderer_passes_the_argument_through of test_depth_alpha_window_cpu /
    test_depth_alpha_tile_cpu and the literals of the callers here); per call the same scalar fields and input pointers of GmpiRenderParams (outputs and the node's
    private T buffer are each run's own) and byte-equal layout structs."""
    assert [c.name for c in a] == [c.name for c in b] and len(a) >= 2
    for ca, cb in zip(a, b):
        assert len(ca.args) == len(cb.args)
        assert scalars_of(ca.args[0]) == scalars_of(cb.args[0]), ca.name
        for k in SAME_POINTERS:
            assert getattr(ca.args[0], k) == getattr(cb.args[0], k), (ca.name, k)
        for i in range(1, 1 + n_structs):
            assert bytes(ca.args[i]) == bytes(cb.args[i]), (ca.name, i)
    fwd = [c for c in a if "backward" not in c.name][-1]
    for i in range(1, 1 + n_structs):   # ... and the backward's are the forward's
        assert bytes(a[-1].args[i]) == bytes(fwd.args[i]), i
    assert [x for x in a[-1].args[1 + n_structs:] if isinstance(x, list)] == [x for x in b[-1].args[1 + n_structs:] if isinstance(x, list)]   # gradient strides


@pytest.mark.parametrize("background", [False, True])
@pytest.mark.parametrize("variant", [None, "gather", "lds"])
def test_shared_colour_reaches_the_c_abi_the_same_through_both_doors(rec2, variant, background):
    """(On host tensors "lds" is not asked of the library -- the staged forward's query, fallback counter and warning need the device:
    tests/test_hip_shared_forward_staged.py -- so that case pins that both doors accept the name and hand over the same AUTO launch.)"""
    from ml_gmpi_amd.hip_mpi import MPI
    rgb, alpha, bg, geo = shared_inputs(background=background)
    r, infos, dhw = renderer_and_cameras(geo)
    kw = {} if variant is None else {"variant": variant}

    def through_mpi():
        res = MPI().render_views_shared(rgb, alpha, dhw, *geo[1:], background=bg, out_pm1=True, check_last_plane=True, want_transmittance=True, **kw)
        return res["color"], res["depth"], res["T"]

    def through_renderer():
        out = r.render_shared(rgb, alpha, H, W, background_rgb=bg, given_cam_infos=infos, want_transmittance=True, **kw)
        return out[0], out[1], out[4]
    a, b = both_doors(rec2, through_mpi, through_renderer, (rgb, alpha, bg), uses_T=background)
    assert_same_calls(a, b, 1)
    assert tuple(c.name for c in a) == SHARED
    assert a[0].args[0].variant == b[0].args[0].variant == (1 if variant == "gather" else 0)   # (host tensors: "lds" is not asked for)


@pytest.mark.parametrize("background", [False, True])
@pytest.mark.parametrize("depth_backward", ["pixel", "tile"])
@pytest.mark.parametrize("depth_forward", ["pixel", "window"])
def test_depth_alpha_reaches_the_c_abi_the_same_through_both_doors(rec2, depth_forward, depth_backward, background):
    from ml_gmpi_amd import depth_alpha_bounds
    from ml_gmpi_amd.hip_mpi import MPI
    rgb, depth, pz, bg, geo = depth_inputs(background=background, per_mpi_table=background)
    r, infos, dhw = renderer_and_cameras(geo)
    kw = dict(depth_forward=depth_forward, depth_backward=depth_backward)

    def through_mpi():
        res = MPI().render_views_depth(rgb, depth, pz, depth_alpha_bounds(1, 4), dhw, *geo[1:], background=bg, out_pm1=True, check_last_plane=True,
                                       want_transmittance=True, **kw)
        return res["color"], res["depth"], res["T"]

    def through_renderer():
        out = r.render_depth(rgb, depth, H, W, z_range=1, n_z_bins=4, plane_z=pz, background_rgb=bg, given_cam_infos=infos, want_transmittance=True, **kw)
        return out[0], out[1], out[4]
    a, b = both_doors(rec2, through_mpi, through_renderer, (rgb, depth, bg), uses_T=not background)
    assert_same_calls(a, b, 2)
    assert a[-1].name == DEPTH_BACKWARD[depth_backward] and len(a) == (3 if depth_forward == "window" else 2)
    assert a[-1].args[2].plane_z == pz.data_ptr()   # (fp32 on the device already: the table itself)


def test_the_removed_private_keywords_are_refused_by_name(rec2):
    """A caller that still passes one must fail loudly, not render the volume path over an alpha tensor."""
    from ml_gmpi_amd.hip_mpi import MPI
    vol, *geo = make_inputs(2)
    r, infos, dhw = renderer_and_cameras(geo)
    for name in REMOVED_KEYWORDS:
        with pytest.raises(TypeError, match=name):
            MPI().render_views(vol, *geo, **{name: None})
        with pytest.raises(AssertionError, match="unknown arguments"):
            r.render(vol, H, W, given_cam_infos=infos, **{name: None})
    assert rec2.calls == []


def test_the_window_fallback_warning_names_the_callers_line(rec2, monkeypatch):
    from ml_gmpi_amd import hip_mpi
    monkeypatch.setattr(hip_mpi, "_WINDOW_FALLBACK_WARNED", False)
    rgb, depth, pz, bg, geo = depth_inputs()
    rec2.answer = 0
    mpi = hip_mpi.MPI()
    with warnings.catch_warnings(record=True) as seen, torch.no_grad():
        warnings.simplefilter("always")
        mpi.render_views_depth(rgb, depth, pz, (-0.2, 0.2), *geo, background=bg, depth_forward="window")
    (w,) = [x for x in seen if issubclass(x.category, RuntimeWarning)]
    assert os.path.samefile(w.filename, __file__) and mpi.depth_window_fallbacks == 1
