"""GPU tests of two small kernels of csrc/gmpi_abi.hip that the render tests reach at one input only.

`gmpi_rgba_range_check_launch` (range_check="full": the reference's min >= 0 / max <= 1 over the WHOLE volume) is an assertion -- a false
negative is silent.  Its work is split four ways: a 16-byte vector kernel whose lanes walk the volume with a 4x unrolled body and a remainder
loop, a scalar launch for the `count % per` elements behind the last full vector, and the scalar kernel alone for a base that is not 16-byte
aligned.  One bad element is planted in every one of those territories (and a clean buffer is checked to stay clean), for counts around every
boundary, in all three storage dtypes; the verdict is always the one numpy gives on the same buffer.

`frames_to_uint8`: values ON the quantisation boundaries, at the clamps, image-only / depth-only / N == 0 / `out=` slices.
Run on the MI355X box:  python -m pytest tests -m gpu"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RANGE_BIT = 2                      # GMPI_STATUS_RGBA_RANGE
BLOCKS_MAX, THREADS = 256 * 8, 256  # the launch of range_check_vec_kernel: min((nvec + 255) / 256, 2048) blocks of 256 lanes
FULL_GRID = BLOCKS_MAX * THREADS

# storage dtype -> (torch dtype, numpy dtype of the host mirror, ABI code, elements per 16-byte vector)
FORMATS = {"f32": (torch.float32, np.float32, 0, 4), "bf16": (torch.bfloat16, np.uint16, 1, 8), "f16": (torch.float16, np.float16, 2, 8)}


def _to_f32(host, fmt):
    """The host mirror as float32 values (bf16 is kept as its 16 bits: numpy has no such type)."""
    if fmt == "bf16":
        return (host.astype(np.uint32) << np.uint32(16)).view(np.float32)
    return host.astype(np.float32)


def _encode(value, fmt):
    """A float32 value that the format holds exactly -> one element of the host mirror."""
    v = np.float32(value)
    if fmt == "bf16":
        bits = np.array([v]).view(np.uint32)[0]
        assert bits & np.uint32(0xFFFF) == 0, value
        return np.uint16(bits >> np.uint32(16))
    out = FORMATS[fmt][1](v)
    assert np.isnan(v) or np.float32(out) == v, value
    return out


def _mirror(values, fmt):
    """float32 values that the format holds exactly -> the host mirror array."""
    if fmt == "f32":
        return values.astype(np.float32)
    if fmt == "f16":
        return values.astype(np.float16)
    return (values.astype(np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def _as_tensor(host, fmt):
    """The host mirror as a CPU tensor of the storage dtype over the same bits."""
    if fmt == "bf16":
        return torch.from_numpy(host.view(np.int16)).view(torch.bfloat16)
    return torch.from_numpy(host)


def _poke(op_dev, op_host, idx, fmt):
    """Copies element idx of the host mirror to the device as it is (bits, no arithmetic)."""
    op_dev[idx:idx + 1].copy_(_as_tensor(op_host[idx:idx + 1].copy(), fmt))


def _specials(fmt):
    """(bad values, good values) as float32 numbers exact in the format: the neighbours of the two bounds, NaN, the infinities, both zeros, the
    smallest subnormal.  `in_unit` is v >= 0 && v <= 1."""
    mant, emin = {"f32": (23, -126), "bf16": (7, -126), "f16": (10, -14)}[fmt]
    eps, tiny, sub = 2.0 ** -mant, 2.0 ** emin, 2.0 ** (emin - mant)
    bad = [1.0 + eps, -tiny, -sub, float("nan"), float("inf"), float("-inf")]     # nextafter(1, 2), -tiny, the negative subnormal, ...
    good = [0.0, 1.0, -0.0, sub, 1.0 - eps / 2]                                      # ... and nextafter(1, 0) on the good side
    return bad, good


def _numpy_verdict(host, fmt):
    v = _to_f32(host, fmt)
    return 0 if bool(((v >= 0) & (v <= 1)).all()) else RANGE_BIT     # (NaN fails both comparisons, as in the kernel)


def _territory(j, nvec):
    """Which loop of range_check_vec_kernel reads vector j of nvec.  The grid has G = min(ceil(nvec / 256), 2048) * 256 lanes; lane g starts at
    i = g and, while i + 3G < nvec, reads i, i + G, i + 2G, i + 3G (the unrolled body) and advances by 4G; what is left it reads one vector per trip
    (the remainder loop).  So vector j belongs to lane g = j % G on trip t = j / G, inside the unrolled group that starts at trip 4 (t / 4) if that
    whole group fits: g + (4 (t / 4) + 3) G < nvec.  (tests/test_light_shapes_cpu.py checks this model against a walk through the two loops.)"""
    G = min((nvec + THREADS - 1) // THREADS, BLOCKS_MAX) * THREADS
    g, t = j % G, j // G
    return "unrolled" if g + (4 * (t // 4) + 3) * G < nvec else "remainder"


def _positions(count, per, aligned):
    """Element indices to plant a bad value at -> {label: index}.  For a misaligned base everything is the scalar kernel's: first, middle, last."""
    pos = {"first": 0, "last": count - 1, "middle": count // 2}
    if not aligned:
        return pos
    nvec, tail = count // per, count % per
    if tail:
        pos["tail first"], pos["tail last"] = nvec * per, count - 1
    if nvec:
        pos["last full vector"] = (nvec - 1) * per + per - 1
        want = {"unrolled", "remainder"}
        for j in sorted({0, nvec // 3, nvec // 2, (2 * nvec) // 3, nvec - 1, max(nvec - 1 - FULL_GRID, 0), max(nvec - 1 - 4 * FULL_GRID, 0)}, reverse=True):
            kind = _territory(j, nvec)
            if kind in want:
                want.discard(kind)
                pos[f"{kind} loop (vector {j})"] = j * per + (j % per)
    return pos


def _counts(per):
    big = (10 * FULL_GRID + 777) * per + (per - 1)     # 10.0015 grids of vectors: two unrolled trips and two or three remainder trips per lane, a full tail
    return [1, per - 1, per, per + 1, 4 * per * 256 - 1, 4 * per * 256, 4 * per * 256 + 1, (4 * FULL_GRID + 5) * per + 1, big]


def _run(lib, dev_buf, code, count, status):
    status.zero_()
    rc = lib.gmpi_rgba_range_check_launch(dev_buf.data_ptr(), code, count, status.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    words = status.cpu().numpy()
    assert not words[1:].any()
    return int(words[0])


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "offset-by-one-element"])
def test_range_check_finds_one_bad_element_wherever_it_is(fmt, aligned):
    from ml_gmpi_amd import _lib
    lib = _lib.load_library()
    tdtype, ndtype, code, per = FORMATS[fmt]
    bad_values, good_values = _specials(fmt)
    status = torch.zeros(_lib.STATUS_WORDS, dtype=torch.int32, device=DEV)
    rng = np.random.default_rng(17)
    big = _counts(per)[-1]
    # one buffer for every count: U[0, 1) values k / 256 (exact in every format), on the host and, the same bits, on the device; buf[off:] is the operand
    off = 0 if aligned else 1
    host = _mirror(rng.integers(0, 256, size=big + off).astype(np.float32) / np.float32(256), fmt)
    dev = _as_tensor(host, fmt).to(DEV)
    assert dev.dtype == tdtype and (dev.data_ptr() + off * dev.element_size()) % 16 == (0 if aligned else dev.element_size())
    op_dev, op_host = dev[off:], host[off:]
    planted = 0
    seen = set()
    for count in _counts(per):
        h = op_host[:count]
        assert _numpy_verdict(h, fmt) == 0 and _run(lib, op_dev, code, count, status) == 0, ("clean", count)
        for label, idx in _positions(count, per, aligned).items():
            seen.add(label.split(" (")[0])
            keep = h[idx].copy()
            values = [(v, True) for v in bad_values] + [(v, False) for v in good_values]
            if count > 64 * per * 256:                      # the two large buffers: one bad and one good value per position, taken in turn
                values = [values[planted % len(bad_values)], values[len(bad_values) + planted % len(good_values)]]
            for value, is_bad in values:
                h[idx] = _encode(value, fmt)
                _poke(op_dev, h, idx, fmt)
                want = _numpy_verdict(h, fmt)               # numpy on the same buffer decides, not this table
                assert want == (RANGE_BIT if is_bad else 0), (value, want)
                got = _run(lib, op_dev, code, count, status)
                assert got == want, (fmt, aligned, count, label, idx, value, got, want)
                planted += 1
            h[idx] = keep
            _poke(op_dev, h, idx, fmt)
        # the element behind the operand's end is not read: a bad value there leaves the verdict clean
        if count < big:
            keep = op_host[count].copy()
            op_host[count] = _encode(float("nan"), fmt)
            _poke(op_dev, op_host, count, fmt)
            assert _run(lib, op_dev, code, count, status) == 0, ("one past the end", count)
            op_host[count] = keep
            _poke(op_dev, op_host, count, fmt)
    # the device buffer is the host mirror again, bit for bit
    back = dev.view(torch.int16).cpu().numpy().view(np.uint16) if fmt == "bf16" else dev.cpu().numpy()
    assert np.array_equal(back.view(np.uint8), host.view(np.uint8))
    want_seen = {"first", "last", "middle"} | ({"tail first", "tail last", "last full vector", "unrolled loop", "remainder loop"} if aligned else set())
    assert seen == want_seen, seen
    print(f"{fmt} {'aligned' if aligned else 'misaligned'}: {planted} planted values, verdicts equal to numpy's")


@pytest.mark.parametrize("where", ["tail", "remainder loop", "unrolled loop"])
def test_mpi_full_range_check_sees_each_territory(where):
    """The same through `MPI(range_check="full")`.  The bad value sits in an MPI that no view renders: range_check="touched" (the texels the
    render samples) stays silent, the exhaustive pass of "full" must raise the reference's assertion wherever it keeps that element."""
    from test_hip_parity import _random_case, hip_render
    if where == "tail":             # 16-bit, 3 MPIs of 3 * 4 * 15 * 15 elements: 8100, not a multiple of 8
        dtype, cfg, per = torch.bfloat16, dict(seed=3, B=3, D=3, S=15), 8
    elif where == "unrolled loop":  # 8 grids of vectors: every lane's two unrolled trips, no remainder
        dtype, cfg, per = torch.float32, dict(seed=4, B=2, D=32, S=256), 4
    else:                           # fewer vectors than lanes: one remainder trip each
        dtype, cfg, per = torch.float32, dict(seed=5, B=2, D=5, S=48), 4
    rgba, dhw, ray, eye, zd = _random_case(**cfg)
    vol = rgba.to(dtype).to(DEV).contiguous()
    count = vol.numel()
    nvec = count // per
    if where == "tail":
        assert count % per
        idx = count - 1
    else:
        idx = (nvec - 1) * per + 1
        assert _territory(nvec - 1, nvec) == where.split()[0]
    assert idx >= count - count // cfg["B"]                   # in the last MPI
    args = (dhw, ray[:1], eye[:1], zd[:1])                    # one view, of MPI 0
    kw = dict(variant="gather", view_to_mpi=[0], check_last=False)
    assert int(hip_render(vol, *args, range_check="full", **kw)["status"][0]) == 0
    vol.view(-1)[idx] = 1.5
    assert int(hip_render(vol, *args, range_check="touched", **kw)["status"][0]) == 0
    with pytest.raises(AssertionError):
        hip_render(vol, *args, range_check="full", **kw)
    torch.cuda.synchronize()


# ---- frames_to_uint8 -----------------------------------------------------------------------------------------------------------------------------
def _numpy_frames(rgb, dep, near, far):
    """render_video.py:118-126, as tests/test_hip_parity.py::test_frames_to_uint8_matches_numpy_recipe; values outside [-1, 1] are clamped before
    the cast (numpy's cast of an out-of-range float is undefined; the kernel clamps to 0 / 255)."""
    img = rgb.transpose(0, 2, 3, 1)
    img = (img + 1) / 2.0
    img8 = np.clip(img * 255, 0, 255).astype(np.uint8)
    if dep is None:
        return img8, None
    d = dep.transpose(0, 2, 3, 1)
    d = (d - near) / (far - near)
    d = np.clip(d, 0, 1)
    return img8, (d * 255).astype(np.uint8)


def _boundary_frames(N, H, W, near, far):
    """Every quantisation boundary k / 127.5 - 1 with its two fp32 neighbours (k = 0 .. 255: 768 values, the outer two beyond the clamps), values
    well outside, and for the depth `near`, `far`, their fp32 neighbours and a ramp over the 256 depth boundaries -- tiled over N frames."""
    k = np.arange(256, dtype=np.float64)
    b = (k / 127.5 - 1.0).astype(np.float32)
    vals = np.concatenate([b, np.nextafter(b, np.float32(-2)), np.nextafter(b, np.float32(2)), np.float32([-1.5, 1.5, -1.0, 1.0, 0.0, -0.0])])
    rgb = np.resize(vals, (N, 3, H, W)).astype(np.float32)
    n32, f32 = np.float32(near), np.float32(far)
    db = (near + (far - near) * k / 255.0).astype(np.float32)
    dv = np.concatenate([db, np.nextafter(db, np.float32(0)), np.nextafter(db, np.float32(9)),
                         np.float32([n32, f32, np.nextafter(n32, np.float32(0)), np.nextafter(f32, np.float32(9)), near - 0.5, far + 0.5])])
    dep = np.resize(dv, (N, 1, H, W)).astype(np.float32)
    assert rgb.size >= vals.size and dep.size >= dv.size
    return rgb, dep


def test_frames_to_uint8_on_quantisation_boundaries_and_clamps():
    from ml_gmpi_amd import frames_to_uint8
    near, far = 0.95, 1.12
    N, H, W = 2, 13, 31                                              # not square, H * W odd
    rgb, dep = _boundary_frames(N, H, W, near, far)
    want, want_d = _numpy_frames(rgb, dep, near, far)
    inside = (rgb >= -1) & (rgb <= 1)                                # there the recipe needs no clamp: (img * 255).astype(np.uint8) as it stands
    plain = (((rgb + 1) / 2.0) * 255).astype(np.uint8)
    assert np.array_equal(plain[inside], want.transpose(0, 3, 1, 2)[inside])
    assert len(np.unique(want)) == 256 and len(np.unique(want_d)) == 256
    img8, dep8 = frames_to_uint8(torch.from_numpy(rgb).to(DEV), torch.from_numpy(dep).to(DEV), near, far)
    torch.cuda.synchronize()
    assert tuple(img8.shape) == (N, H, W, 3) and tuple(dep8.shape) == (N, H, W, 1) and img8.dtype == dep8.dtype == torch.uint8
    assert np.array_equal(img8.cpu().numpy(), want), np.argwhere(img8.cpu().numpy() != want)[:5]
    assert np.array_equal(dep8.cpu().numpy(), want_d), np.argwhere(dep8.cpu().numpy() != want_d)[:5]
    # image only
    only, none = frames_to_uint8(torch.from_numpy(rgb).to(DEV), None, near, far)
    assert none is None and np.array_equal(only.cpu().numpy(), want)
    # `out=`: slices of a path-long buffer, the frames around them stay as they were
    buf = torch.full((N + 3, H, W, 3), 77, dtype=torch.uint8, device=DEV)
    dbuf = torch.full((N + 3, H, W, 1), 78, dtype=torch.uint8, device=DEV)
    a, b = frames_to_uint8(torch.from_numpy(rgb).to(DEV), torch.from_numpy(dep).to(DEV), near, far, out=(buf[1:1 + N], dbuf[2:2 + N]))
    torch.cuda.synchronize()
    assert a.data_ptr() == buf[1:].data_ptr() and b.data_ptr() == dbuf[2:].data_ptr()
    assert np.array_equal(buf[1:1 + N].cpu().numpy(), want) and np.array_equal(dbuf[2:2 + N].cpu().numpy(), want_d)
    assert bool((buf[0] == 77).all()) and bool((buf[1 + N:] == 77).all()) and bool((dbuf[:2] == 78).all()) and bool((dbuf[2 + N:] == 78).all())


def test_frames_to_uint8_depth_only_and_no_frames():
    from ml_gmpi_amd import _lib, frames_to_uint8
    lib = _lib.load_library()
    near, far = 0.95, 1.12
    N, H, W = 3, 17, 18
    rgb, dep = _boundary_frames(N, H, W, near, far)
    _, want_d = _numpy_frames(rgb, dep, near, far)
    dep_d = torch.from_numpy(dep).to(DEV)
    dep8 = torch.full((N, H, W, 1), 9, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.gmpi_frames_to_uint8_launch(None, dep_d.data_ptr(), N, H, W, near, far, None, dep8.data_ptr(), stream) == 0   # depth only
    torch.cuda.synchronize()
    assert np.array_equal(dep8.cpu().numpy(), want_d)
    # N == 0: nothing is launched, nothing written; neither through the entry nor through the wrapper
    dep8.fill_(9)
    assert lib.gmpi_frames_to_uint8_launch(None, dep_d.data_ptr(), 0, H, W, near, far, None, dep8.data_ptr(), stream) == 0
    assert lib.gmpi_frames_to_uint8_launch(None, None, N, H, W, near, far, None, None, stream) == 0                        # no output asked for
    assert lib.gmpi_frames_to_uint8_launch(None, dep_d.data_ptr(), N, H, W, near, far, dep8.data_ptr(), None, stream) == -1  # an image without its source
    assert lib.gmpi_frames_to_uint8_launch(None, None, N, H, W, near, far, None, dep8.data_ptr(), stream) == -1
    assert lib.gmpi_frames_to_uint8_launch(None, dep_d.data_ptr(), N, 0, W, near, far, None, dep8.data_ptr(), stream) == -2
    torch.cuda.synchronize()
    assert bool((dep8 == 9).all())
    img8, d8 = frames_to_uint8(torch.empty((0, 3, H, W), device=DEV), torch.empty((0, 1, H, W), device=DEV), near, far)
    assert tuple(img8.shape) == (0, H, W, 3) and tuple(d8.shape) == (0, H, W, 1)
