"""`install()` swaps the reference's MPI / MPIRenderer for the HIP ones.  What the reference hands this package at its seams -- the arguments
of `MPI(...)` and `MPI.forward` from its MPIRenderer, the `render()` calls of its video driver -- was recorded by running the reference
(oracle/make_golden.py seams -> tests/golden/reference_seams.npz) and is replayed here; stand-in `gmpi.core.*` modules (empty classes, no
reference code) are what install() patches.  No kernel is launched here."""
import contextlib
import io
import sys
import types

import pytest
import torch

from _util import load_npz

SEAMS = load_npz("reference_seams.npz")


@pytest.fixture
def reference_modules(monkeypatch):
    """`gmpi.core.mpi` / `gmpi.core.mpi_renderer` / `gmpi.core.light_renderer` as install() finds them: the names it rebinds, bound to
    placeholders."""
    mods = {n: types.ModuleType(n) for n in ("gmpi", "gmpi.core", "gmpi.core.mpi", "gmpi.core.mpi_renderer", "gmpi.core.light_renderer")}
    mpi_cls = type("MPI", (), {})
    mods["gmpi.core.mpi"].MPI = mpi_cls
    mods["gmpi.core.mpi_renderer"].MPI = mpi_cls                       # mpi_renderer.py imports the name
    mods["gmpi.core.mpi_renderer"].MPIRenderer = type("MPIRenderer", (), {})
    mods["gmpi.core.light_renderer"].LightRenderer = type("LightRenderer", (), {})   # train.py:23 imports the name
    mods["gmpi"].core = mods["gmpi.core"]
    for name in ("mpi", "mpi_renderer", "light_renderer"):
        setattr(mods["gmpi.core"], name, mods[f"gmpi.core.{name}"])
    for name, m in mods.items():
        monkeypatch.setitem(sys.modules, name, m)
    return types.SimpleNamespace(mpi=mods["gmpi.core.mpi"], mpi_renderer=mods["gmpi.core.mpi_renderer"],
                                 light_renderer=mods["gmpi.core.light_renderer"])


def _recorded_kwargs(prefix):
    """The keyword arguments of a recorded call, rebuilt as the reference passed them (lists of per-view tensors where it passed lists)."""
    kw = {}
    for key, kind in SEAMS["meta"][prefix]["kwargs"].items():
        name = key[len(prefix) + 1:]
        if kind == "tensor":
            kw[name] = torch.from_numpy(SEAMS[key])
        elif kind == "tensor_list":
            kw[name] = list(torch.from_numpy(SEAMS[key]).unbind(0))
        elif kind == "number_list":
            kw[name] = SEAMS[key].tolist()
        else:
            kw[name] = kind["value"]
    return kw


def test_install_patches_the_reference_modules_and_uninstall_restores(reference_modules):
    ns = reference_modules
    import ml_gmpi_amd
    orig_mpi, orig_renderer, orig_light = ns.mpi.MPI, ns.mpi_renderer.MPIRenderer, ns.light_renderer.LightRenderer
    try:
        ml_gmpi_amd.install()
        import gmpi.core.mpi as m
        import gmpi.core.mpi_renderer as mr
        assert issubclass(m.MPI, ml_gmpi_amd.MPI) and mr.MPI is m.MPI and issubclass(mr.MPIRenderer, ml_gmpi_amd.MPIRenderer)
        assert m.MPI.DEFAULT_RANGE_CHECK == "full" and ml_gmpi_amd.MPI.DEFAULT_RANGE_CHECK == "touched"   # no process-global default
        # the way render_video.py binds the name (`from gmpi.core.mpi_renderer import MPIRenderer`) after install()
        from gmpi.core.mpi_renderer import MPIRenderer
        assert issubclass(MPIRenderer, ml_gmpi_amd.MPIRenderer)
        from gmpi.core.light_renderer import LightRenderer          # train.py:23
        assert LightRenderer is ml_gmpi_amd.LightRenderer
    finally:
        ml_gmpi_amd.uninstall()
    assert ns.mpi.MPI is orig_mpi and ns.mpi_renderer.MPIRenderer is orig_renderer and ns.light_renderer.LightRenderer is orig_light


def test_reference_renderer_with_patched_mpi_keeps_its_geometry(reference_modules):
    """patch_renderer=False: the reference's own MPIRenderer constructs our MPI through its seam (mpi_renderer.py:47) with the recorded
    arguments, and its plane geometry (recorded) is ours bit for bit."""
    import ml_gmpi_amd
    ctor = SEAMS["meta"]["ctor"]
    try:
        ml_gmpi_amd.install(patch_renderer=False)
        mpi = reference_modules.mpi_renderer.MPI(**ctor["kwargs"])
        assert isinstance(mpi, ml_gmpi_amd.MPI) and mpi._align_corners is True
        ours = ml_gmpi_amd.make_renderer(ctor["preset"], n_planes=ctor["D"], device=torch.device("cpu"))
        assert torch.equal(torch.from_numpy(SEAMS["ctor_static_dhws"]), ours.static_mpi_plane_dhws)
    finally:
        ml_gmpi_amd.uninstall()


class _RecordingLibrary:
    """Stands in for libgmpi_render.so: every launch records a copy of its arguments and returns GMPI_OK."""
    records_only = True

    def __init__(self):
        self.calls = []

    def _copy_params(self, pref):
        import ctypes
        from ml_gmpi_amd import _lib
        src = ctypes.cast(pref, ctypes.POINTER(_lib.GmpiRenderParams)).contents
        dst = _lib.GmpiRenderParams()
        ctypes.memmove(ctypes.byref(dst), ctypes.byref(src), ctypes.sizeof(dst))
        return dst

    def gmpi_mpi_render_launch(self, pref, stream):
        self.calls.append(("render", self._copy_params(pref), stream))
        return 0

    def gmpi_rgba_range_check_launch(self, ptr, dtype, count, status, stream):
        self.calls.append(("range_check", (ptr, dtype, count, status), stream))
        return 0


def test_reference_render_drives_the_hip_mpi_through_its_seam(monkeypatch, reference_modules):
    """The reference's OWN `MPIRenderer.render` (mpi_renderer.py:387-469) with only `MPI` swapped: the call at
    mpi_renderer.py:451-461 (keyword arguments, per-view lists, c2w_mat, sphere_c -- recorded from the reference, replayed here as its
    `self.mpi(...)` makes it) must reach `MPI.forward` and be marshalled into the GmpiRenderParams the C ABI expects.  The library is
    replaced by a recorder (no GPU needed)."""
    import ml_gmpi_amd
    from ml_gmpi_amd import _lib
    rec = _RecordingLibrary()
    monkeypatch.setattr(_lib, "load_library", lambda: rec)
    seen = {}
    orig_forward = ml_gmpi_amd.MPI.forward

    def spy(self, **kw):
        seen.update(kw)
        return orig_forward(self, **kw)

    monkeypatch.setattr(ml_gmpi_amd.MPI, "forward", spy)
    fwd = SEAMS["meta"]["fwd"]
    B, D, S, T = fwd["B"], fwd["D"], fwd["S"], fwd["T"]
    try:
        ml_gmpi_amd.install(patch_renderer=False)        # default: the reference's whole-volume range assertion
        mpi = reference_modules.mpi_renderer.MPI(**SEAMS["meta"]["ctor"]["kwargs"])   # mpi_renderer.py:47
        assert isinstance(mpi, ml_gmpi_amd.MPI) and mpi.range_check == "full"
        rgb, depth = mpi(**_recorded_kwargs("fwd"))
    finally:
        ml_gmpi_amd.uninstall()
    assert ml_gmpi_amd.MPI.DEFAULT_RANGE_CHECK == "touched"
    # what the reference passed through the seam (mpi_renderer.py:451-461)
    assert set(seen) == {"batch_rgba", "batch_dhw", "batch_ray_dir", "batch_eye_pos", "batch_z_dir", "separate_background",
                         "assert_not_out_of_last_plane", "c2w_mat", "sphere_c"}
    assert seen["separate_background"] is None and seen["assert_not_out_of_last_plane"] is True
    assert len(seen["batch_ray_dir"]) == B and tuple(seen["batch_ray_dir"][0].shape) == (1, 3, S, S)
    assert tuple(seen["c2w_mat"].shape) == (B, 4, 4) and len(seen["sphere_c"]) == 3
    # what reached the C ABI: the exhaustive range check first, then ONE render launch
    assert [c[0] for c in rec.calls] == ["range_check", "render"]
    ptr, dtype, count, status_ptr = rec.calls[0][1]
    assert dtype == _lib.DTYPE_F32 and count == B * D * 4 * T * T
    p = rec.calls[1][1]
    assert (p.N, p.M, p.D, p.Ht, p.Wt, p.H, p.W, p.views_per_mpi) == (B, B, D, T, T, S, S, 1)
    assert p.view_to_mpi is None and p.rgba == ptr and p.status == status_ptr
    assert list(p.rgba_stride) == [D * 4 * T * T, 4 * T * T, T * T, T, 1]
    assert p.rgba_dtype == _lib.DTYPE_F32 and p.variant == _lib.VARIANT_AUTO
    # MPI.forward returns colour in [0,1]: the reference applies 2c-1 itself (mpi_renderer.py:467), so OUT_PM1 is off
    assert p.flags == (_lib.FLAG_ALIGN_CORNERS | _lib.FLAG_CHECK_LAST_PLANE | _lib.FLAG_CHECK_RANGE)
    assert p.transmittance_out is None and p.rgb_out and p.depth_out
    assert tuple(rgb.shape) == (B, 3, S, S) and tuple(depth.shape) == (B, 1, S, S)
    assert p.rgb_out == rgb.data_ptr() and p.depth_out == depth.data_ptr()


class _EyeRecordingLibrary(_RecordingLibrary):
    """Also keeps the eye positions the launch was given (the tensors are alive during the call)."""

    def gmpi_mpi_render_launch(self, pref, stream):
        import ctypes
        p = self._copy_params(pref)
        eye = (ctypes.c_float * (3 * p.N)).from_address(p.eye_pos)
        self.calls.append(("render", p, list(eye)))
        return 0


def test_reference_generate_img_drives_the_installed_renderer(monkeypatch, reference_modules):
    """The reference's video driver -- `generate_img` (gmpi/eval/vis/render_video.py:19-132) -- after `install()`: the renderer it builds is
    the installed one (`from gmpi.core.mpi_renderer import MPIRenderer`, constructed and set up as render_video.py:168-205 does), and the
    calls it makes to `render()` for a path of 5 camera angles (recorded from the reference with a fake generator standing in for the
    StyleGAN2 network) are replayed; the library is a recorder (no GPU needed).  Every camera angle of the path must arrive at the C ABI as
    ONE render launch of the generator's volume, with the pose the angle asks for (h_mean = angle, stddev 0: render_video.py:100-113, 236-237)."""
    import ml_gmpi_amd
    from ml_gmpi_amd import _lib
    from ml_gmpi_amd.poses import gen_sphere_path
    rec = _EyeRecordingLibrary()
    monkeypatch.setattr(_lib, "load_library", lambda: rec)
    video = SEAMS["meta"]["video"]
    D, S, T = video["D"], video["S"], video["T"]
    angles = video["angles"]
    assert video["generator_calls"] == [D, D] and len(video["calls"]) == len(angles)   # (the reference's own flow, as recorded)
    vol = torch.from_numpy(SEAMS["video_rgba"])
    outs = []
    try:
        ml_gmpi_amd.install()
        from gmpi.core.mpi_renderer import MPIRenderer                # render_video.py:11, bound AFTER install()
        assert issubclass(MPIRenderer, ml_gmpi_amd.MPIRenderer)
        kw = dict(video["renderer_kwargs"], device=torch.device("cpu"))
        with contextlib.redirect_stdout(io.StringIO()):
            renderer = MPIRenderer(**kw)                              # as render_video.py:168-189
            renderer.get_xyz_interpolate_ws(D, D)                     # :193
            renderer.set_cam(kw["cam_fov"], S, S)                     # :198
            renderer.get_xyz(T, T, ret_single_res=False, only_z=False)   # :200-205
        for call in video["calls"]:                                   # :107-116
            outs.append(renderer.render(vol, *call["size"], **call["kwargs"]))
    finally:
        ml_gmpi_amd.uninstall()
    renders = [c for c in rec.calls if c[0] == "render"]
    assert len(renders) == len(angles) == len(outs)
    assert [c["kwargs"]["horizontal_mean"] for c in video["calls"]] == pytest.approx(angles, abs=0)
    # install(): the reference's whole-volume assertion (mpi_renderer.py:447-449) -- ONCE for the loop's one unchanged volume (round 6; rounds 1-5 paid the
    # exhaustive pass in front of every one of the path's views: tests/test_range_check_cache.py)
    assert [c[0] for c in rec.calls] == ["range_check", "render"] + ["render"] * (len(angles) - 1)
    for (_, p, eye), yaw in zip(renders, angles):
        assert (p.N, p.M, p.D, p.Ht, p.Wt, p.H, p.W) == (1, 1, D, T, T, S, S)
        assert p.flags & _lib.FLAG_OUT_PM1 and p.flags & _lib.FLAG_CHECK_LAST_PLANE and p.variant == _lib.VARIANT_AUTO
        assert p.rgba == vol.data_ptr()
        c2w, yaws, pitches = gen_sphere_path(n_cams=1, sphere_center=renderer.sphere_center, sphere_r=renderer.sphere_r, yaw_mean=yaw,
                                             yaw_std=0.0, pitch_mean=0.0, pitch_std=0.0, n_truncated_stds=renderer.cam_pose_n_truncated_stds,
                                             flag_rnd=True, sample_method=renderer.cam_sample_method, given_yaws=None, given_pitches=None)
        want = torch.as_tensor(c2w)[0, :3, 3].float().tolist()
        assert eye == pytest.approx(want, abs=0), (yaw, eye, want)
    img, depth, _, _ = outs[0]
    assert tuple(img.shape) == (1, 3, S, S) and tuple(depth.shape) == (1, 1, S, S)
