"""Host side of the detector's letterbox (kasportsformer_amd.letterbox_frames, kasf_letterbox_plan / kasf_letterbox_frames): the numpy restatement of
include/kasf.h's rules 1-4 that the GPU test and the host-compiled kernel test hold the kernel to (both import ``letterbox_np`` from here), tied to what the
reference's own letterbox_image / prep_image wrote into the fixture (tests/golden/make_letterbox_golden.py: their bookkeeping around a stand-in cv2.resize),
and checked on every pixel against exact fp64 cubic convolution; the refusals of both entry points and of the Python surface.  cv2.resize itself could not
be recorded (no OpenCV build at hand): rules 2-3 are tested as a resampling scheme with a stated error bound, not as "the bits of cv2"."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32, F64, I64 = np.float32, np.float64, np.int64
ODD_SIZES = [(64, 64), (33, 31), (5, 3), (12, 8), (48, 32)]            # (out_w, out_h) the kernel tests share: four-pixel stores, element stores, non-square


def fixture():
    return np.load(os.path.join(GOLDEN, "letterbox.npz"), allow_pickle=False)


def fixture_frame(fx, name):
    """Fixture frame ``name`` ('land': 97 x 131, smooth; 'port': 131 x 97, noise) as a [Hf,Wf,3] uint8 VIEW of its pitched buffer [Hf,pitch] (padding bytes are 255)."""
    buf = fx[name + "_buf"]
    Hf, Wf = (int(v) for v in fx[name + "_hw"])
    return np.lib.stride_tricks.as_strided(buf, shape=(Hf, Wf, 3), strides=(buf.strides[0], 3, 1), writeable=False)


def plan_np(Wf, Hf, out_w, out_h):
    """Rule 1 in Python floats, as letterbox_image writes it -> (new_w, new_h, pad_x, pad_y)."""
    new_w = int(Wf * min(out_w / Wf, out_h / Hf))
    new_h = int(Hf * min(out_w / Wf, out_h / Hf))
    return new_w, new_h, (out_w - new_w) // 2, (out_h - new_h) // 2


def cubic_table_np(n_src, n_dst):
    """Rule 2 for one axis -> (s [n_dst] int64, a [n_dst,4] int64): tap k of position d is source index clamp(s[d] - 1 + k), weight a[d, k] / 2048."""
    scale = F64(1.0) / (F64(n_dst) / F64(n_src))
    f = ((np.arange(n_dst, dtype=F64) + 0.5) * scale - 0.5).astype(F32)
    fl = np.floor(f)
    t = f - fl
    A, one = F32(-0.75), F32(1)
    u, w = t + one, one - t
    c = np.stack((((A * u - F32(5) * A) * u + F32(8) * A) * u - F32(4) * A,
                  ((A + F32(2)) * t - (A + F32(3))) * t * t + one,
                  ((A + F32(2)) * w - (A + F32(3))) * w * w + one), axis=-1)
    c = np.concatenate((c, (one - c[:, 0] - c[:, 1] - c[:, 2])[:, None]), axis=-1)
    assert f.dtype == t.dtype == c.dtype == F32
    a = np.rint(c * F32(2048)).astype(I64)
    assert np.abs(a).max() <= 32767
    return fl.astype(I64), a


def resize_cubic_np(src, new_w, new_h, stats=None):
    """Rules 2-3: src [Hf,Wf,C] uint8 -> [new_h,new_w,C] uint8, horizontal pass then vertical pass in int64 (equal to the 16-tap form: the sums are exact)."""
    src = np.asarray(src)
    Hf, Wf = src.shape[:2]
    sx, a = cubic_table_np(Wf, new_w)
    sy, b = cubic_table_np(Hf, new_h)
    cols = np.clip(sx[:, None] - 1 + np.arange(4), 0, Wf - 1)
    rows = np.clip(sy[:, None] - 1 + np.arange(4), 0, Hf - 1)
    s64 = src.astype(I64)
    h = sum(a[None, :, k, None] * s64[:, cols[:, k]] for k in range(4))                 # [Hf, new_w, C]
    V = sum(b[:, k, None, None] * h[rows[:, k]] for k in range(4))                      # [new_h, new_w, C]
    assert np.abs(V).max() < 2 ** 31, "rule 3: V fits 32 bits"
    if stats is not None:
        stats["V"] = max(stats.get("V", 0), int(np.abs(V).max()))
    return np.clip((V + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


def letterbox_np(frame, inp_dim, pad=128, swap_rb=True, parts=False):
    """kasf_letterbox_frames restated: frame [Hf,Wf,3] or [F,Hf,Wf,3] uint8, inp_dim = int or (width, height) -> float32 [F,3,out_h,out_w] ([1,...] for one
    frame); with parts=True also the uint8 canvases [F,out_h,out_w,3] before rule 4."""
    frame = np.asarray(frame)
    frames = frame if frame.ndim == 4 else frame[None]
    out_w, out_h = (inp_dim, inp_dim) if isinstance(inp_dim, int) else inp_dim
    Hf, Wf = frames.shape[1:3]
    new_w, new_h, pad_x, pad_y = plan_np(Wf, Hf, out_w, out_h)
    assert new_w >= 1 and new_h >= 1
    canvas = np.full((len(frames), out_h, out_w, 3), pad, np.uint8)
    for f, img in enumerate(frames):
        canvas[f, pad_y:pad_y + new_h, pad_x:pad_x + new_w] = resize_cubic_np(img, new_w, new_h)
    planes = canvas[..., ::-1] if swap_rb else canvas
    out = np.ascontiguousarray(planes.transpose(0, 3, 1, 2)).astype(F32) / F32(255)
    assert out.dtype == F32
    return (out, canvas) if parts else out


def exact_cubic_np(src, new_w, new_h, A=-0.75, centre=0.5):
    """Cubic convolution in fp64: positions (d + 0.5) n_src / n_dst - 0.5, Keys' kernel with A, replicated edge, clamped to [0, 255] -> float64 [new_h,new_w,C]."""
    def axis(n_src, n_dst):
        p = (np.arange(n_dst, dtype=F64) + centre) * n_src / n_dst - centre
        s = np.floor(p)
        t = p - s
        w = np.stack((((A * (t + 1) - 5 * A) * (t + 1) + 8 * A) * (t + 1) - 4 * A, ((A + 2) * t - (A + 3)) * t * t + 1,
                      ((A + 2) * (1 - t) - (A + 3)) * (1 - t) * (1 - t) + 1), axis=-1)
        w = np.concatenate((w, 1 - w.sum(axis=-1, keepdims=True)), axis=-1)
        return np.clip(s.astype(I64)[:, None] - 1 + np.arange(4), 0, n_src - 1), w
    src = np.asarray(src).astype(F64)
    cols, wx = axis(src.shape[1], new_w)
    rows, wy = axis(src.shape[0], new_h)
    h = sum(wx[None, :, k, None] * src[:, cols[:, k]] for k in range(4))
    return np.clip(sum(wy[:, k, None, None] * h[rows[:, k]] for k in range(4)), 0.0, 255.0)


def noise_frame(Hf, Wf, seed, binary=False):
    g = np.random.default_rng(seed)
    return (g.integers(0, 2, (Hf, Wf, 3)) * 255 if binary else g.integers(0, 256, (Hf, Wf, 3))).astype(np.uint8)


def lib_plan(Wf, Hf, out_w, out_h):
    """kasf_letterbox_plan -> (code, (new_w, new_h, pad_x, pad_y))."""
    from kasportsformer_amd import _lib
    v = [C.c_int32(-7) for _ in range(4)]
    code = _lib.load().kasf_letterbox_plan(Wf, Hf, out_w, out_h, *(C.byref(x) for x in v))
    return code, tuple(x.value for x in v)


def test_fixture_loads_without_pickles_and_is_small():
    path = os.path.join(GOLDEN, "letterbox.npz")
    assert os.path.getsize(path) < 200 * 1024
    fx = fixture()
    assert tuple(fx["land_hw"]) == (97, 131) and tuple(fx["port_hw"]) == (131, 97)
    for name in ("land", "port"):
        buf, (Hf, Wf) = fx[name + "_buf"], fx[name + "_hw"]
        assert buf.dtype == np.uint8 and buf.shape[0] == Hf and buf.shape[1] > 3 * Wf and (buf[:, 3 * Wf:] == 255).all(), "the padding of the pitch is marked"
    diff = lambda f: int(max(np.abs(np.diff(f.astype(I64), axis=0)).max(), np.abs(np.diff(f.astype(I64), axis=1)).max()))
    assert diff(fixture_frame(fx, "land")) <= 16 < diff(fixture_frame(fx, "port")), "a smooth frame and a noisy one"
    assert int(fx["interpolation"]) == 2 and fx["dsize"].shape == (len(fx["calls"]), 2) and fx["placement"].shape == (len(fx["calls"]), 4)


def test_restatement_equals_the_reference_bookkeeping_bit_for_bit():
    """prep_image and letterbox_image as the reference wrote them (around the stand-in resize): new_w / new_h, placement, the 128 canvas, the channel reversal,
    the layout and float().div(255.0)."""
    fx = fixture()
    for name in ("land", "port"):
        for dim in (64, 32):
            want = fx[f"{name}_prep_{dim}"]
            got = letterbox_np(fixture_frame(fx, name), dim)
            assert want.dtype == F32 and want.shape == (1, 3, dim, dim) and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, dim)
    canvas = fx["land_canvas_48x32"]
    got, parts = letterbox_np(fixture_frame(fx, "land"), (48, 32), parts=True)
    assert canvas.shape == (32, 48, 3) and np.array_equal(parts[0], canvas)
    assert np.array_equal(got[0], (canvas[:, :, ::-1].transpose(2, 0, 1).astype(F32) / F32(255)))


def test_plan_equals_the_recorded_sizes_and_the_python_expression():
    fx = fixture()
    shapes = {"land": (131, 97), "port": (97, 131)}
    for call, dsize, place in zip(fx["calls"], fx["dsize"], fx["placement"]):
        name, w, h = str(call).split(":")
        Wf, Hf = shapes[name]
        code, (new_w, new_h, pad_x, pad_y) = lib_plan(Wf, Hf, int(w), int(h))
        assert code == 0 and (new_w, new_h) == tuple(dsize) and (pad_x, pad_y, new_w, new_h) == tuple(place), call
        assert (new_w, new_h, pad_x, pad_y) == plan_np(Wf, Hf, int(w), int(h))
    g = np.random.default_rng(416)
    seen = 0
    for Wf, Hf, out_w, out_h in zip(g.integers(1, 32768, 2000), g.integers(1, 32768, 2000), g.integers(1, 4097, 2000), g.integers(1, 4097, 2000)):
        Wf, Hf, out_w, out_h = int(Wf), int(Hf), int(out_w), int(out_h)
        if g.random() < 0.5:                                                     # near-square frames and the exact-ratio cases as well
            Hf = max(1, min(32767, Wf * out_h // out_w + int(g.integers(-1, 2))))
        want = plan_np(Wf, Hf, out_w, out_h)
        code, got = lib_plan(Wf, Hf, out_w, out_h)
        if want[0] < 1 or want[1] < 1:
            assert code == 2, (Wf, Hf, out_w, out_h)
        else:
            assert code == 0 and got == want, (Wf, Hf, out_w, out_h, got, want)
            assert 0 <= got[2] and got[2] + got[0] <= out_w and 0 <= got[3] and got[3] + got[1] <= out_h
            seen += 1
    assert seen >= 1500
    assert lib_plan(1920, 1080, 416, 416) == (0, (416, 234, 0, 91))


ACCURACY = [(5, 7, 8), (5, 7, 3), (30, 40, 96), (97, 131, 64), (131, 97, 32), (240, 320, 416), (1080, 1920, 416)]         # Hf, Wf, inp_dim


def test_scheme_is_cubic_convolution_within_the_stated_bound():
    """Every output pixel of every case against exact fp64 cubic convolution (A = -0.75, half-pixel centres, replicated edge, clamped): at most 1.25 grey levels =
    0.5 (final rounding) + 0.69 (11-bit coefficients: 255 * 2^-12 * 4 * 1.375 per pass) + 0.03 (fp32 position at coordinates up to 1920), kasf.h.  On the noise
    frame a kernel with A = -0.5 or without the half-pixel centre is far outside the bound."""
    worst, stats = 0.0, {}
    for Hf, Wf, dim in ACCURACY:
        new_w, new_h, _, _ = plan_np(Wf, Hf, dim, dim)
        for binary in (False, True):
            frame = noise_frame(Hf, Wf, seed=Hf + dim, binary=binary)
            v = resize_cubic_np(frame, new_w, new_h, stats).astype(F64)
            err = float(np.abs(v - exact_cubic_np(frame, new_w, new_h)).max())
            worst = max(worst, err)
            assert err <= 1.25, (Hf, Wf, dim, binary, err)
    frame = noise_frame(97, 131, seed=1)
    v = resize_cubic_np(frame, 64, 47).astype(F64)
    other_a = float(np.abs(v - exact_cubic_np(frame, 64, 47, A=-0.5)).max())
    no_centre = float(np.abs(v - exact_cubic_np(frame, 64, 47, centre=0.0)).max())
    print(f"fixed-point vs exact cubic convolution: worst {worst:.3f} grey levels (bound 1.25); largest |V| {stats['V']:.3e} (< 2^31 = 2.147e9); "
          f"against A = -0.5: {other_a:.1f}, against no half-pixel centre: {no_centre:.1f}")
    assert other_a > 5 and no_centre > 5, "the bound tells these apart"


def test_identity_when_nothing_is_resized():
    frame = noise_frame(64, 64, seed=3)
    assert plan_np(64, 64, 64, 64) == (64, 64, 0, 0)
    out, canvas = letterbox_np(frame, 64, parts=True)
    assert np.array_equal(canvas[0], frame), "t = 0 everywhere: weights 0, 2048, 0, 0"
    assert np.array_equal(out[0], frame[:, :, ::-1].transpose(2, 0, 1).astype(F32) / F32(255))


def test_tiny_frames_where_every_tap_clamps():
    """1 x 1: every tap is the one pixel p, so V = p * sum(a) * sum(b); the sums are 2048 give or take 1 (measured over every table of this file's cases), which
    moves v by at most 255 * 2 / 2048 = 0.25 < 0.5: the result is p itself, and the restatement gives exactly that."""
    for Hf, Wf, dim in ACCURACY + [(1, 1, 8), (3, 2, 8), (5, 7, 12)]:
        new_w, new_h, _, _ = plan_np(Wf, Hf, dim, dim)
        for n_src, n_dst in ((Wf, new_w), (Hf, new_h)):
            assert np.abs(cubic_table_np(n_src, n_dst)[1].sum(axis=1) - 2048).max() <= 1
    for p in (0, 1, 77, 128, 254, 255):
        frame = np.array([[[p, 255 - p, (p * 7) % 256]]], np.uint8)
        out, canvas = letterbox_np(frame, 8, parts=True)
        assert (canvas[0] == frame[0, 0]).all() and out.shape == (1, 3, 8, 8), p
    for Hf, Wf in ((3, 2), (5, 7)):
        frame = noise_frame(Hf, Wf, seed=Hf)
        for dim in (8, (12, 8), 3):
            out, canvas = letterbox_np(frame, dim, parts=True)
            assert np.isfinite(out).all() and out.min() >= 0 and out.max() <= 1
            new_w, new_h, pad_x, pad_y = plan_np(Wf, Hf, *((dim, dim) if isinstance(dim, int) else dim))
            inside = np.zeros(canvas.shape[1:3], bool)
            inside[pad_y:pad_y + new_h, pad_x:pad_x + new_w] = True
            assert (canvas[0][~inside] == 128).all()
    assert plan_np(2, 3, 8, 8) == (5, 8, 1, 0)
    assert (letterbox_np(np.full((3, 2, 3), 200, np.uint8), 8, parts=True)[1][0][:, 1:6] == 200).all(), "a flat frame stays flat, for the same reason"


def entry_args():
    """Host buffers and the argument list of kasf_letterbox_frames for one 5 x 7 frame into 6 x 4 -> (call, buffers)."""
    from kasportsformer_amd import _lib
    lib = _lib.load()
    frame, out = np.full(2 * 5 * 7 * 3, 3, np.uint8), np.full(2 * 3 * 4 * 6, 7, F32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(frames=vp(frame), n_frames=1, Hf=5, Wf=7, row_stride=21, frame_stride=105, out=vp(out), dtype=0, out_w=6, out_h=4, pad=128, swap=1):
        return lib.kasf_letterbox_frames(frames, n_frames, Hf, Wf, row_stride, frame_stride, out, dtype, out_w, out_h, pad, swap, None)

    return call, (frame, out)


REFUSED = [dict(n_frames=-1), dict(Hf=0), dict(Wf=0), dict(Hf=-1), dict(Hf=32768), dict(Wf=32768, row_stride=3 * 32768), dict(out_w=0), dict(out_h=0),
           dict(out_w=-3), dict(out_w=4097), dict(out_h=4097), dict(row_stride=20), dict(row_stride=0), dict(row_stride=-21), dict(frame_stride=-1),
           dict(frame_stride=-105, n_frames=2), dict(n_frames=2, frame_stride=104), dict(n_frames=2, frame_stride=0), dict(dtype=3), dict(dtype=-1),
           dict(pad=-1), dict(pad=256), dict(Hf=1, Wf=32767, row_stride=3 * 32767, frame_stride=3 * 32767), dict(Hf=32767, Wf=1, row_stride=3, frame_stride=3 * 32767),
           dict(frames=None), dict(out=None)]
PLAN_REFUSED = [(0, 5, 6, 4), (7, 0, 6, 4), (-7, 5, 6, 4), (32768, 5, 6, 4), (7, 32768, 6, 4), (7, 5, 0, 4), (7, 5, 6, 0), (7, 5, 4097, 4), (7, 5, 6, 4097), (7, 5, -6, 4),
                (32767, 1, 6, 4), (1, 32767, 416, 416), (4097, 1, 4096, 4096)]


def test_entry_points_refuse_without_a_device():
    from kasportsformer_amd import _lib
    lib = _lib.load()
    for name in ("kasf_letterbox_plan", "kasf_letterbox_frames"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    hdr = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "kasf.h")).read()
    assert "int kasf_letterbox_plan(int32_t Wf, int32_t Hf, int32_t out_w, int32_t out_h, int32_t* new_w, int32_t* new_h, int32_t* pad_x, int32_t* pad_y);" in hdr
    assert "int kasf_letterbox_frames(const void* frames, int32_t n_frames, int32_t Hf, int32_t Wf, int64_t row_stride, int64_t frame_stride, void* out, int32_t out_dtype," in hdr
    assert "equality with a particular cv2 build is not verified" in hdr and "#define KASF_LETTERBOX_MAX_SIDE 4096" in hdr
    assert _lib.ABI_VERSION == lib.kasf_version() == 12
    for args in PLAN_REFUSED:
        code, got = lib_plan(*args)
        assert code == 2 and got == (-7, -7, -7, -7) and lib.kasf_last_error(), args
    v = C.c_int32(-7)
    for hole in range(4):
        ptrs = [None if i == hole else C.byref(v) for i in range(4)]
        assert lib.kasf_letterbox_plan(7, 5, 6, 4, *ptrs) == 2 and v.value == -7
    assert lib_plan(7, 5, 6, 4) == (0, (5, 4, 0, 0)) and lib_plan(32767, 8, 4096, 4096) == (0, plan_np(32767, 8, 4096, 4096))
    call, (frame, out) = entry_args()
    assert call(n_frames=0) == 0 and call(frames=None, out=None, n_frames=0) == 0                 # nothing to do
    for kw in REFUSED:
        assert call(**kw) == 2, kw
        assert lib.kasf_last_error(), kw
    assert (frame == 3).all() and (out == 7).all(), "a refused call touches no buffer"


def test_python_surface_refuses_before_any_launch():
    import kasportsformer_amd as K
    from kasportsformer_amd.letterbox import check_letterbox_args, letterbox_plan
    assert "letterbox_frames" in K.__all__ and "LetterboxResult" in K.__all__ and "letterbox_frames" in K.__doc__
    assert "NOT verified" in K.letterbox.__doc__ and "not verified against a cv2 build" in K.letterbox_frames.__doc__
    frame = np.zeros((9, 11, 3), np.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.letterbox_frames(frame, 8, device="cpu")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            K.letterbox_frames(frame)
        with pytest.raises(RuntimeError, match="no CPU path"):
            K.letterbox_frames(torch.zeros((2, 9, 11, 3), dtype=torch.uint8), (12, 8), pad=0, swap_rb=False, dtype=torch.bfloat16)
    f = K.letterbox_frames
    for exc, call in ((TypeError, lambda: f(frame.astype(F32))),
                      (TypeError, lambda: f(frame.tolist())),
                      (TypeError, lambda: f(torch.zeros((9, 11, 3)))),
                      (TypeError, lambda: f(frame, 8.0)),
                      (TypeError, lambda: f(frame, "416")),
                      (TypeError, lambda: f(frame, (8, 8, 8))),
                      (TypeError, lambda: f(frame, (8.5, 8))),
                      (TypeError, lambda: f(frame, True)),
                      (TypeError, lambda: f(frame, None)),
                      (TypeError, lambda: f(frame, 8, pad=128.0)),
                      (TypeError, lambda: f(frame, 8, pad=None)),
                      (TypeError, lambda: f(frame, 8, dtype=torch.float64)),
                      (TypeError, lambda: f(frame, 8, dtype=np.float32)),
                      (ValueError, lambda: f(frame[:, :, :2])),
                      (ValueError, lambda: f(frame[0])),
                      (ValueError, lambda: f(frame[None][:0])),
                      (ValueError, lambda: f(frame[:0])),
                      (ValueError, lambda: f(frame, 0)),
                      (ValueError, lambda: f(frame, -416)),
                      (ValueError, lambda: f(frame, 4097)),
                      (ValueError, lambda: f(frame, (8, 0))),
                      (ValueError, lambda: f(frame, (4097, 8))),
                      (ValueError, lambda: f(frame, 8, pad=-1)),
                      (ValueError, lambda: f(frame, 8, pad=256)),
                      (ValueError, lambda: f(np.zeros((1, 4000, 3), np.uint8), 416)),          # new_h = 0: the reference's cv2.resize raises
                      (ValueError, lambda: f(np.zeros((2, 4000, 1, 3), np.uint8), (416, 8)))):
        with pytest.raises(exc):
            call()
    assert not frame.any()
    fr, size, pad, new, off = check_letterbox_args(frame, (12, 8), 7, torch.float16, "t")
    assert fr.shape == (9, 11, 3) and size == (12, 8) and pad == 7 and (new, off) == ((9, 8), (1, 0)) == letterbox_plan(11, 9, 12, 8)
    assert check_letterbox_args(frame, np.int64(8), np.uint8(0), torch.float32, "t")[1:3] == ((8, 8), 0)
