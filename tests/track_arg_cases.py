"""Every refusal the lifting, tracked and filter surfaces raise about their track, slot and stream arguments, as a table of refused Python calls
(tests/test_track_args_cpu.py replays it against tests/golden/track_arg_refusals.json; tests/golden/make_track_arg_golden.py recorded that file).

A case is ``(call, case id, thunk)``: ``call`` is the ``who`` its message begins with, the thunk makes the call.  No case needs a device, and none behaves
differently where one is present: the model is a stub that says it lives on cuda:0, the objects are made without their allocating constructors, a tensor "on
another GPU" is a host tensor whose class says cuda:1, and a tensor on the wrong kind of device is a ``meta`` one.  A case named ``a+b`` holds two faults; its
record is that of the check that comes first, which is what moving checks into shared helpers can change unnoticed.
"""
import ast
import os
import pickle
import sys
import tempfile
from types import SimpleNamespace

import numpy as np
import torch

import kasportsformer_amd as K
from kasportsformer_amd import bones, lift, smooth, stream, tracked

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "track_arg_refusals.json")
MODULES = ("lift.py", "stream.py", "tracked.py", "smooth.py", "bones.py", "_tracks.py")        # whose every raise the table must reach (those that exist)
CUDA0 = torch.device("cuda", 0)

# (module, a piece of the raise statement's source, why no case reaches it): at most 10 % of the raises
UNREACHED = [
    ("lift.py", '"lift_track: width and height must be positive"', "lift_track uploads the track before it looks at the resolution: it needs a device"),
    ("lift.py", "window count disagrees with window_plan", "needs a library that disagrees with the host plan, and a device behind it"),
    ("lift.py", "window plan disagrees with ragged_plan", "needs a library that disagrees with the host plan, and a device behind it"),
    ("stream.py", "window tables disagree with stream_tables", "needs a library that disagrees with the host tables"),
]


class Elsewhere(torch.Tensor):
    """A host tensor that says it is on a second GPU (no machine of the CPU tests has two)."""
    is_cuda = True
    device = torch.device("cuda", 1)


def elsewhere(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype).as_subclass(Elsewhere)


def f32(*shape):
    return np.zeros(shape, np.float32)


def meta(*shape, dtype=torch.int32):
    return torch.empty(shape, dtype=dtype, device="meta")


def bare(cls, **attrs):
    o = object.__new__(cls)
    o.__dict__.update(attrs)
    return o


MODEL = SimpleNamespace(_flat=SimpleNamespace(device=CUDA0), n_frames=27, training=False)
HOST_MODEL = SimpleNamespace(_flat=SimpleNamespace(device=torch.device("cpu")), n_frames=27, training=False)
KP, F64 = f32(5, 17, 3), np.zeros((5, 17, 3), np.float64)
T_OK = SimpleNamespace(ids=meta(2, 4), slot=meta(2, 4), born=meta(2, 4), count=meta(2))


def tr(**kw):
    return SimpleNamespace(**dict(vars(T_OK), **kw))


def streamer(**kw):
    return bare(K.StreamLifter, **dict(dict(device=CUDA0, slots=4, T=27, lag=2, flip=True, layout="h36m", _coco=False, _one_resolution=None,
                                            _counts=np.array([3, 0, 3, 3], np.int64), model=MODEL), **kw))


def tracker(**kw):
    return bare(K.TrackedLifter, **dict(dict(device=CUDA0, streams=2, track_slots=4, R=2, T=27, lag=0, flip=True, _coco=False, model=MODEL), **kw))


def euro(**kw):
    return bare(K.OneEuroFilter, **dict(dict(tracked=False, slots=4, joints=17, channels=2, _Ct=3, score=True, streams=None, track_slots=None, R=None,
                                             device=CUDA0, tick=0), **kw))


def boner(**kw):
    return bare(K.BoneLengthFilter, **dict(dict(tracked=False, slots=4, streams=None, track_slots=None, R=None, device=CUDA0, window=8, symmetric=False), **kw))


TRACKED = dict(tracked=True, slots=8, streams=2, track_slots=4, R=2)
HM, CS = f32(4, 17, 8, 8), f32(4, 2)


def keypoint_file(obj, name):
    """load_keypoints of a pickle of obj, from a relative path so that the message does not depend on where the file is."""
    here = os.getcwd()
    with tempfile.TemporaryDirectory() as d:
        os.chdir(d)
        try:
            with open(name, "wb") as f:
                f.write(obj if isinstance(obj, bytes) else pickle.dumps(obj))
            return lift.load_keypoints(name)
        finally:
            os.chdir(here)


def _lift_cases():
    lt, lts = "lift_track", "lift_tracks"
    yield "window_plan", "T", lambda: lift.window_plan(5, 0)
    yield "window_plan", "stride", lambda: lift.window_plan(5, 4, 5)
    yield "window_plan", "n", lambda: lift.window_plan(-1, 4)
    yield "window_plan", "ragged:T", lambda: lift.ragged_plan([3], 0)
    yield "keypoint file", "global", lambda: keypoint_file(b"cos\nsystem\n(S'true'\ntR.", "kp.pkl")
    yield "kp.pkl", "not_numeric", lambda: keypoint_file([1], "kp.pkl")
    yield lt, "layout", lambda: K.lift_track(MODEL, KP, 1280, 720, layout="mpii")
    yield lt, "layout+model", lambda: K.lift_track(HOST_MODEL, KP, 1280, 720, layout="mpii")
    yield lt, "model", lambda: K.lift_track(HOST_MODEL, KP, 1280, 720)
    yield lt, "model+dtype", lambda: K.lift_track(HOST_MODEL, F64, 1280, 720)
    yield lt, "dtype_np", lambda: K.lift_track(MODEL, F64, 1280, 720)
    yield lt, "dtype_torch", lambda: K.lift_track(MODEL, torch.zeros((5, 17, 3), dtype=torch.float16), 1280, 720)
    yield lt, "other_gpu", lambda: K.lift_track(MODEL, elsewhere(5, 17, 3), 1280, 720)
    yield lt, "meta", lambda: K.lift_track(MODEL, torch.zeros((5, 17, 3), device="meta"), 1280, 720)
    yield lt, "not_array", lambda: K.lift_track(MODEL, [[0.0]], 1280, 720)
    yield lt, "shape", lambda: K.lift_track(MODEL, f32(5, 17, 2), 1280, 720)
    yield lt, "dtype+shape", lambda: K.lift_track(MODEL, np.zeros((5, 17, 2)), 1280, 720)
    yield lt, "shape+stride", lambda: K.lift_track(MODEL, f32(5, 17, 2), 1280, 720, stride=0)
    for k, bad in (("model", HOST_MODEL), ("stride", None)):
        yield lts, "layout+" + k, lambda bad=bad: K.lift_tracks(bad or MODEL, [KP], 1280, 720, layout="mpii", stride=0)
    yield lts, "model", lambda: K.lift_tracks(HOST_MODEL, [KP], 1280, 720)
    yield lts, "stride", lambda: K.lift_tracks(MODEL, [KP], 1280, 720, stride=28)
    yield lts, "max_windows", lambda: K.lift_tracks(MODEL, [KP], 1280, 720, max_windows=0)
    yield lts, "stride+dtype", lambda: K.lift_tracks(MODEL, [F64], 1280, 720, stride=0)
    yield lts, "dtype", lambda: K.lift_tracks(MODEL, [KP, F64], 1280, 720)
    yield lts, "dtype_torch", lambda: K.lift_tracks(MODEL, [torch.zeros((5, 17, 3), dtype=torch.float64)], 1280, 720)
    yield lts, "other_gpu", lambda: K.lift_tracks(MODEL, [KP, elsewhere(5, 17, 3)], 1280, 720)
    yield lts, "meta", lambda: K.lift_tracks(MODEL, [torch.zeros((5, 17, 3), device="meta")], 1280, 720)
    yield lts, "not_array", lambda: K.lift_tracks(MODEL, [KP, "x"], 1280, 720)
    yield lts, "shape", lambda: K.lift_tracks(MODEL, [KP, KP[0]], 1280, 720)
    yield lts, "shape4", lambda: K.lift_tracks(MODEL, [KP[None]], 1280, 720)
    yield lts, "dtype_of_2nd+shape_of_1st", lambda: K.lift_tracks(MODEL, [KP[0], F64], 1280, 720)       # every part is converted before any shape is looked at
    yield lts, "shape+width", lambda: K.lift_tracks(MODEL, [KP[..., :2]], -1, 720)
    yield lts, "width_count", lambda: K.lift_tracks(MODEL, [KP, KP], [1280, 1280, 1280], 720)
    yield lts, "width_sign", lambda: K.lift_tracks(MODEL, [KP], 1280, 0)
    yield lts, "width+height", lambda: K.lift_tracks(MODEL, [KP], [1, 2], [3, 4, 5])
    yield lts, "packed_dtype", lambda: K.lift_tracks(MODEL, F64, 1280, 720, offsets=[0, 5])
    yield lts, "packed_shape", lambda: K.lift_tracks(MODEL, KP[None], 1280, 720, offsets=[0, 5])
    yield lts, "packed_list", lambda: K.lift_tracks(MODEL, [KP], 1280, 720, offsets=[0, 5])
    yield lts, "packed_dtype+shape", lambda: K.lift_tracks(MODEL, F64[0], 1280, 720, offsets=[0, 5])
    yield lts, "packed_shape+offsets", lambda: K.lift_tracks(MODEL, KP[0], 1280, 720, offsets=[1, 5])
    for k, off in (("end", [0, 4]), ("start", [1, 5]), ("descending", [0, 3, 2, 5]), ("float", [0.0, 5.0]), ("empty", []), ("2d", [[0, 5]]),
                   ("tensor", torch.tensor([0, 6]))):
        yield lts, "offsets_" + k, lambda off=off: K.lift_tracks(MODEL, KP, 1280, 720, offsets=off)
    yield lts, "offsets+width", lambda: K.lift_tracks(MODEL, KP, [1, 2, 3], 720, offsets=[0, 4])
    yield lts, "packed_width_count", lambda: K.lift_tracks(MODEL, KP, [1, 2, 3], 720, offsets=[0, 2, 5])
    yield lts, "stride+offsets", lambda: K.lift_tracks(MODEL, KP, 1280, 720, offsets=[0, 4], stride=0)


def _stream_cases():
    S = "StreamLifter"
    yield "stream_tables", "T", lambda: stream.stream_tables(0)
    yield S, "layout", lambda: K.StreamLifter(MODEL, 1280, 720, layout="mpii")
    yield S, "layout+model", lambda: K.StreamLifter(HOST_MODEL, 1280, 720, layout="mpii")
    yield S, "model+slots", lambda: K.StreamLifter(HOST_MODEL, 1280, 720, slots=0)
    yield S, "slots+lag", lambda: K.StreamLifter(MODEL, 1280, 720, slots=0, lag=27)
    yield S, "lag+width", lambda: K.StreamLifter(MODEL, [1, 2], 720, slots=4, lag=27)
    yield S, "width_count", lambda: K.StreamLifter(MODEL, [1, 2], 720, slots=4)
    yield S, "height_sign", lambda: K.StreamLifter(MODEL, 1280, -720, slots=4)
    for who, call in ((S + ".push", lambda s, ids: s.push(f32(2, 17, 3), slots=ids)), (S + ".tail", lambda s, ids: s.tail(slots=ids)),
                      (S + ".reset", lambda s, ids: s.reset(slots=ids)),
                      (S + ".push_heatmaps", lambda s, ids: s.push_heatmaps(HM[:2], CS[:2], CS[:2], slots=ids))):
        for k, ids in (("2d", [[0, 1]]), ("float", [0.0, 1.0]), ("high", [0, 4]), ("negative", [-1, 0]), ("twice", [1, 1]), ("twice+range", [5, 5]),
                       ("tensor", torch.tensor([0, 7])), ("on_gpu", elsewhere(2, dtype=torch.int64))):
            yield who, "slots_" + k, lambda call=call, ids=ids: call(streamer(), ids)
    p = S + ".push"
    yield p, "dtype", lambda: streamer().push(F64[:4])
    yield p, "other_gpu", lambda: streamer().push(elsewhere(4, 17, 3))
    yield p, "meta", lambda: streamer().push(torch.zeros((4, 17, 3), device="meta"))
    yield p, "not_array", lambda: streamer().push(None)
    yield p, "dtype+slots", lambda: streamer().push(F64[:4], slots=[9])
    yield p, "slots+shape", lambda: streamer().push(KP, slots=[9])
    yield p, "shape_all", lambda: streamer().push(KP)
    yield p, "shape_some", lambda: streamer().push(KP, slots=[0, 1])
    yield p, "shape_joints", lambda: streamer().push(f32(4, 17, 2))
    ph = S + ".push_heatmaps"
    yield ph, "count", lambda: streamer().push_heatmaps(HM[:3], CS[:3], CS[:3])
    yield ph, "count_some", lambda: streamer().push_heatmaps(HM, CS, CS, slots=[0, 1])
    yield ph, "one_map", lambda: streamer().push_heatmaps(HM[0], CS[0], CS[0])
    yield ph, "decode+slots", lambda: streamer().push_heatmaps(HM, CS, CS, decode="sharp", slots=[9])
    yield ph, "slots+count", lambda: streamer().push_heatmaps(HM[:3], CS[:3], CS[:3], slots=[9])
    yield ph, "other_gpu", lambda: streamer().push_heatmaps(elsewhere(4, 17, 8, 8), CS, CS)
    yield ph, "other_gpu_center", lambda: streamer().push_heatmaps(HM, elsewhere(4, 2), CS)
    yield ph, "count+other_gpu", lambda: streamer().push_heatmaps(elsewhere(3, 17, 8, 8), CS[:3], CS[:3])
    t = S + ".tail"
    yield t, "no_frames", lambda: streamer().tail()
    yield t, "no_frames_some", lambda: streamer().tail(slots=[0, 1])
    yield t, "slots+no_frames", lambda: streamer().tail(slots=[1, 1])
    r = S + ".replay"
    yield r, "dtype", lambda: streamer().replay(F64)
    yield r, "other_gpu", lambda: streamer().replay(elsewhere(5, 17, 3))
    yield r, "shape", lambda: streamer().replay(KP[0])
    yield r, "shape5", lambda: streamer().replay(KP[None, None])
    yield r, "dtype+shape", lambda: streamer().replay(F64[0])
    yield r, "shape+width_alone", lambda: streamer().replay(KP[0], width=1280)
    yield r, "width_alone", lambda: streamer().replay(KP, width=1280)
    yield r, "height_alone", lambda: streamer().replay(KP, height=720)
    yield r, "no_resolution", lambda: streamer().replay(KP)


def _tracked_cases():
    TL = "TrackedLifter"
    good = dict(T=27, width=1280, height=720, streams=2, track_slots=4, rows="persons", num_person=2, lag=0, layout="h36m")

    def args(**kw):
        return lambda: tracked.check_tracked_args(**dict(good, **kw))
    yield TL, "model", lambda: K.TrackedLifter(HOST_MODEL, 1280, 720, layout="mpii")
    yield TL, "layout", lambda: K.TrackedLifter(MODEL, 1280, 720, layout="mpii", rows="people")
    yield TL, "rows+T", args(rows="people", T=0)
    yield TL, "T+streams", args(T=0, streams=0)
    yield TL, "streams_low", args(streams=0, track_slots=0)
    yield TL, "streams_type", args(streams=2.0)
    yield TL, "streams_bool", args(streams=True)
    yield TL, "track_slots_high", args(track_slots=65, num_person=0)
    yield TL, "num_person_low", args(num_person=0, lag=27)
    yield TL, "num_person_high", args(num_person=65536)
    yield TL, "lag_high", args(lag=27, width=[1, 2, 3])
    yield TL, "lag_type", args(lag=None)
    yield TL, "width_count", args(width=[1, 2, 3])
    yield TL, "height_sign", args(height=[720, 0])
    r = TL + ".reset"
    for k, v in (("float", 0.5), ("2d", [[0]]), ("str", "a"), ("high", 2), ("negative", [-1, 0]), ("both", [-1, 2])):
        yield r, "streams_" + k, lambda v=v: tracker().reset(streams=v)
    p = TL + ".push"
    kp = f32(2, 2, 17, 3)
    yield p, "dtype", lambda: tracker().push(np.zeros((2, 2, 17, 3)), T_OK)
    yield p, "other_gpu", lambda: tracker().push(elsewhere(4, 17, 3), T_OK)
    yield p, "meta", lambda: tracker().push(torch.zeros((4, 17, 3), device="meta"), T_OK)
    yield p, "not_array", lambda: tracker().push(None, T_OK)
    yield p, "dtype+shape", lambda: tracker().push(np.zeros((2, 3, 17, 3)), T_OK)
    yield p, "shape", lambda: tracker().push(f32(2, 3, 17, 3), T_OK)
    yield p, "shape_flat", lambda: tracker().push(f32(5, 17, 3), T_OK)
    yield p, "shape+track", lambda: tracker().push(f32(2, 3, 17, 3), object())
    yield p, "no_result", lambda: tracker().push(kp, object())
    yield p, "none", lambda: tracker().push(kp, None)
    yield p, "count_list", lambda: tracker().push(kp, tr(count=[1, 2]))
    yield p, "born_dtype", lambda: tracker().push(kp, tr(born=meta(2, 4, dtype=torch.int64)))
    yield p, "ids_shape", lambda: tracker().push(kp, tr(ids=meta(2, 5)))
    yield p, "slot_shape", lambda: tracker().push(kp, tr(slot=meta(1, 4)))
    yield p, "count_shape", lambda: tracker().push(kp, tr(count=meta(3)))
    yield p, "ids_dtype+slot_shape", lambda: tracker().push(kp, tr(ids=meta(2, 4, dtype=torch.int64), slot=meta(1, 4)))
    yield p, "ids_shape+slot_dtype", lambda: tracker().push(kp, tr(ids=meta(2, 5), slot=meta(2, 4, dtype=torch.int64)))
    yield p, "device", lambda: tracker().push(kp, T_OK)
    yield p, "device_host", lambda: tracker().push(kp, SimpleNamespace(**{k: torch.zeros(v.shape, dtype=torch.int32) for k, v in vars(T_OK).items()}))
    ph = TL + ".push_heatmaps"
    yield ph, "count", lambda: tracker().push_heatmaps(HM[:3], CS[:3], CS[:3], T_OK)
    yield ph, "count5", lambda: tracker().push_heatmaps(f32(2, 3, 17, 8, 8), f32(2, 3, 2), f32(2, 3, 2), T_OK)
    yield ph, "decode+count", lambda: tracker().push_heatmaps(HM[:3], CS[:3], CS[:3], T_OK, decode="sharp")
    yield ph, "count+no_track", lambda: tracker().push_heatmaps(HM[:3], CS[:3], CS[:3])
    yield ph, "no_track", lambda: tracker().push_heatmaps(HM, CS, CS)
    yield ph, "no_result", lambda: tracker().push_heatmaps(HM, CS, CS, object())
    yield ph, "ids_shape", lambda: tracker().push_heatmaps(HM, CS, CS, tr(ids=meta(2, 5)))
    yield ph, "device", lambda: tracker().push_heatmaps(HM, CS, CS, T_OK)
    yield ph, "track+other_gpu", lambda: tracker().push_heatmaps(elsewhere(4, 17, 8, 8), CS, CS, tr(ids=meta(2, 5)))
    yield ph, "other_gpu", lambda: tracker(device=torch.device("meta")).push_heatmaps(elsewhere(4, 17, 8, 8), CS, CS, T_OK)


def _filter_cases(who, make, rows_kw):
    """What OneEuroFilter and BoneLengthFilter refuse alike: the constructor's shape words, reset, and push."""
    for k, kw in (("neither", dict()), ("both", dict(slots=4, streams=1)), ("both_slots", dict(slots=4, track_slots=4)), ("slots_low", dict(slots=0)),
                  ("slots_float", dict(slots=4.0)), ("slots_bool", dict(slots=True)), ("rows", dict(streams=1, track_slots=4, rows="people")),
                  ("rows+streams", dict(streams=0, track_slots=4, rows="people")), ("streams_low", dict(streams=0, track_slots=0)),
                  ("streams_str", dict(streams="1", track_slots=4)), ("track_slots_low", dict(streams=1, track_slots=0)),
                  ("track_slots_high", dict(track_slots=65, num_person=0)), ("num_person_low", dict(streams=1, num_person=0)),
                  ("num_person_tracks", dict(streams=1, rows="tracks", num_person=0)), ("both+rows", dict(slots=4, streams=1, rows="people")),
                  ("shape+device", dict(slots=0, device="cpu")), ("device", dict(slots=4, device="cpu"))):
        yield who, k, lambda kw=kw: make(**kw)
    new = euro if who == "OneEuroFilter" else boner
    r = who + ".reset"
    yield r, "streams_on_slots", lambda: new().reset(streams=[0])
    yield r, "streams_on_slots+slots", lambda: new().reset(slots=[9], streams=[0])
    yield r, "slots_on_tracked", lambda: new(**TRACKED).reset(slots=[0])
    yield r, "slots_on_tracked+streams", lambda: new(**TRACKED).reset(slots=[0], streams=[2])
    for k, v in (("float", 0.5), ("2d", [[0]]), ("str", "a"), ("high", 2), ("negative", [-1]), ("both", [-3, 5])):
        yield r, "streams_" + k, lambda v=v: new(**TRACKED).reset(streams=v)
    for k, v in (("2d", [[0, 1]]), ("float", [0.0]), ("high", [4]), ("negative", [-1, 0]), ("twice", [1, 1]), ("twice+range", [9, 9]),
                 ("tensor", torch.tensor([0, 7])), ("str", ["a"]), ("on_gpu", elsewhere(2, dtype=torch.int64))):
        yield r, "slots_" + k, lambda v=v: new().reset(slots=v)
    p = who + ".push"
    x = f32(4, 17, 3)
    yield p, "dtype", lambda: new().push(x.astype(np.float64))
    yield p, "dtype_torch", lambda: new().push(torch.zeros((4, 17, 3), dtype=torch.bfloat16))
    yield p, "not_array", lambda: new().push([[0.0]])
    yield p, "meta", lambda: new().push(torch.zeros((4, 17, 3), device="meta"))
    yield p, "other_gpu", lambda: new().push(elsewhere(4, 17, 3))
    yield p, "other_gpu+track", lambda: new().push(elsewhere(4, 17, 3), T_OK)
    yield p, "track_on_slots", lambda: new().push(x, T_OK)
    yield p, "track_on_slots+slots", lambda: new().push(x, T_OK, slots=[9])
    for k, v in (("2d", [[0, 1]]), ("float", [0.0, 1.0]), ("high", [0, 4]), ("negative", [-1, 0]), ("twice", [1, 1]), ("on_gpu", elsewhere(2, dtype=torch.int64))):
        yield p, "slots_" + k, lambda v=v: new().push(x[:2], slots=v)
    yield p, "slots+shape", lambda: new().push(x[:3], slots=[0, 4])
    yield p, "shape_all", lambda: new().push(x[:3])
    yield p, "shape_some", lambda: new().push(x, slots=[0, 1])
    yield p, "shape_joints", lambda: new().push(f32(4, 16, 3))
    yield p, "shape_channels", lambda: new().push(x[..., :2])
    yield p, "shape4", lambda: new().push(x[..., None])
    yield p, "dtype+slots_on_tracked", lambda: new(**TRACKED).push(x.astype(np.float64), T_OK, slots=[0])
    yield p, "slots_on_tracked", lambda: new(**TRACKED).push(x, T_OK, slots=[0])
    yield p, "slots_on_tracked+shape", lambda: new(**TRACKED).push(x[:2], T_OK, slots=[0])
    yield p, "tracked_shape", lambda: new(**TRACKED).push(f32(2, 17, 3), T_OK)
    yield p, "tracked_shape4", lambda: new(**TRACKED).push(f32(2, 3, 17, 3), T_OK)
    yield p, "tracked_shape+no_track", lambda: new(**TRACKED).push(f32(2, 3, 17, 3))
    yield p, "no_track", lambda: new(**TRACKED).push(f32(2, 2, 17, 3))
    yield p, "no_result", lambda: new(**TRACKED).push(x, object())
    yield p, "ids_shape", lambda: new(**TRACKED).push(x, tr(ids=meta(2, 5)))
    yield p, "born_dtype", lambda: new(**TRACKED).push(x, tr(born=meta(2, 4, dtype=torch.int64)))
    yield p, "born_dtype+count_shape", lambda: new(**TRACKED).push(x, tr(born=meta(2, 4, dtype=torch.int64), count=meta(3)))
    yield p, "device", lambda: new(**TRACKED).push(x, T_OK)
    for k, kw in rows_kw:
        yield p, k, lambda kw=kw: new().push(x, **kw)


def _smooth_cases():
    who = "OneEuroFilter"
    yield from _filter_cases(who, K.OneEuroFilter, (("ticks_low", dict(ticks=0)), ("ticks_float", dict(ticks=1.0)), ("ticks_bool", dict(ticks=True)),
                                                    ("ticks+slots", dict(ticks=0, slots=[9]))))
    yield who + ".push", "dtype+ticks", lambda: euro().push(F64[:4], ticks=0)
    yield who + ".push", "ticks+slots_on_tracked", lambda: euro(**TRACKED).push(f32(4, 17, 3), T_OK, slots=[0], ticks=0)
    for k, kw in (("joints_low", dict(joints=0)), ("joints_high", dict(joints=257, channels=0)), ("channels_high", dict(channels=5, score=1)),
                  ("channels_float", dict(channels=2.0)), ("score", dict(score=1)), ("score+neither", dict(score=1, slots=None)),
                  ("shape+params", dict(slots=0, rate=0)), ("params+device", dict(beta=-1.0, device="cpu"))):
        yield who, k, lambda kw=kw: K.OneEuroFilter(**dict(dict(slots=4), **kw))
    for w, call in ((who, lambda **kw: K.OneEuroFilter(slots=4, **kw)), ("smooth_tracks", lambda **kw: K.smooth_tracks(KP, **kw))):
        for k, kw in (("rate_zero", dict(rate=0)), ("rate_nan", dict(rate=float("nan"))), ("rate_inf", dict(rate=float("inf"))), ("rate_high", dict(rate=1e7)),
                      ("rate_low", dict(rate=1e-7)), ("rate_str", dict(rate="30")), ("rate_bool", dict(rate=True)), ("beta_none+rate", dict(beta=None, rate=0)),
                      ("min_cutoff_low", dict(min_cutoff=0.0)), ("min_cutoff_nan", dict(min_cutoff=float("nan"))), ("d_cutoff_high", dict(d_cutoff=2e6)),
                      ("rate+min_cutoff", dict(rate=1e7, min_cutoff=0.0)), ("min_cutoff+d_cutoff", dict(min_cutoff=0.0, d_cutoff=0.0)),
                      ("d_cutoff+beta", dict(d_cutoff=0.0, beta=-0.1)), ("beta_low", dict(beta=-0.1)), ("beta_high", dict(beta=2e6)),
                      ("beta_nan+min_score", dict(beta=float("nan"), min_score=float("nan"))), ("min_score_inf+max_hold", dict(min_score=float("inf"), max_hold=-1)),
                      ("max_hold_low", dict(max_hold=-1)), ("max_hold_high", dict(max_hold=2 ** 20 + 1)), ("max_hold_float", dict(max_hold=1.5)),
                      ("max_hold_bool", dict(max_hold=True))):
            yield w, k, lambda call=call, kw=kw: call(**kw)
    st = "smooth_tracks"

    def s(a, **kw):
        return lambda: K.smooth_tracks(a, **kw)
    yield st, "rate+score", s(KP, rate=0.0, score=1)
    yield st, "score", s(KP, score=1)
    yield st, "score+dtype", s(F64, score=1)
    yield st, "dtype", s(F64)
    yield st, "str", s("x")
    yield st, "dtype_in_list", s([KP, KP.astype(np.float16)])
    yield st, "meta", s(torch.zeros((5, 17, 3), device="meta"))
    yield st, "dims_low", s(KP[0])
    yield st, "dims_low_in_list", s([KP, KP[0]])
    yield st, "dims_low_of_1st+dtype_of_2nd", s([KP[0], F64])                 # a part is converted and counted before the next is looked at
    yield st, "dims_high_in_list", s([KP[None]])
    yield st, "dims_high", s(f32(1, 1, 5, 17, 3))
    yield st, "dims_high_packed", s(KP[None], offsets=[0, 5])
    yield st, "dims_high+mixed", s([KP[None], KP[..., :2]])
    yield st, "mixed", s([KP, KP[..., :2]])
    yield st, "mixed_joints+range", s([f32(5, 300, 3), KP])
    yield st, "channels_high", s(f32(5, 17, 6))
    yield st, "channels_high_no_score", s(f32(5, 17, 5), score=False)
    yield st, "channels_low", s(f32(5, 17, 1))
    yield st, "joints_high", s(f32(5, 300, 3))
    yield st, "range+offsets", s(f32(5, 300, 3), offsets=[0, 4])
    for k, off in (("end", [0, 4]), ("start", [1, 5]), ("descending", [0, 3, 2, 5]), ("float", [0.0, 5.0]), ("empty", []), ("tensor", torch.tensor([0, 6]))):
        yield st, "offsets_" + k, s(KP, offsets=off)
    yield st, "offsets+device", s(KP, offsets=[0, 4], device="cpu")
    yield st, "device", s(KP, device="cpu")
    yield st, "device_list", s([KP, KP], device="cpu")
    yield st, "device_4d", s(KP[None], device="cpu")
    yield st, "mixed+device", s([KP, KP[..., :2]], device="cpu")


def _bones_cases():
    who = "BoneLengthFilter"
    yield from _filter_cases(who, K.BoneLengthFilter, ())
    for k, kw in (("window_low", dict(window=0)), ("window_high", dict(window=2 ** 20 + 1)), ("window_float", dict(window=1.5)), ("window_bool", dict(window=True)),
                  ("shape+window", dict(slots=0, window=0)), ("window+symmetric", dict(window=0, symmetric=0)), ("symmetric", dict(symmetric=0)),
                  ("symmetric+device", dict(symmetric=None, device="cpu"))):
        yield who, k, lambda kw=kw: K.BoneLengthFilter(**dict(dict(slots=4), **kw))
    big = torch.zeros(1).expand(2 ** 31, 17, 3)                    # 2^31 frames that take no memory
    for w, call in (("fix_bone_lengths", K.fix_bone_lengths), ("bone_lengths", K.bone_lengths)):
        def b(a, call=call, **kw):
            return lambda: call(a, **kw)
        yield w, "dtype", b(F64)
        yield w, "str", b("x")
        yield w, "meta", b(torch.zeros((5, 17, 3), device="meta"))
        yield w, "dims_low", b(KP[0])
        yield w, "joints", b(f32(5, 16, 3))
        yield w, "channels_in_list", b([KP, KP[..., :2]])
        yield w, "shape_of_1st+dtype_of_2nd", b([KP[0], F64])
        yield w, "dims_high_in_list", b([KP[None]])
        yield w, "dims_high", b(f32(1, 1, 5, 17, 3))
        yield w, "dims_high_packed", b(KP[None], offsets=[0, 5])
        yield w, "dims_high+offsets", b(KP[None], offsets=[0, 4])
        for k, off in (("end", [0, 4]), ("start", [1, 5]), ("descending", [0, 3, 2, 5]), ("float", [0.0, 5.0]), ("empty", []), ("tensor", torch.tensor([0, 6]))):
            yield w, "offsets_" + k, b(KP, offsets=off)
        yield w, "frames", b(big)
        yield w, "frames_packed", b(big, offsets=[0, 2 ** 31])
        yield w, "offsets+device", b(KP, offsets=[0, 4], device="cpu")
        yield w, "frames+device", b(big, device="cpu")
        yield w, "device", b(KP, device="cpu")
        yield w, "device_list", b([KP, KP], device="cpu")
    fx = "fix_bone_lengths"

    def f(a, **kw):
        return lambda: K.fix_bone_lengths(a, **kw)
    yield fx, "shape+symmetric", f(KP[0], symmetric=1)
    yield fx, "offsets+symmetric", f(KP, offsets=[0, 4], symmetric=1)
    yield fx, "frames+symmetric", f(big, symmetric=1)
    yield fx, "symmetric", f(KP, symmetric=1)
    yield fx, "symmetric+return_lengths", f(KP, symmetric=1, return_lengths=None)
    yield fx, "return_lengths", f(KP, return_lengths=0)
    yield fx, "return_lengths+lengths", f(KP, return_lengths=0, lengths=f32(15))
    yield fx, "symmetric+lengths", f(KP, symmetric="yes", lengths=f32(15))
    yield fx, "lengths_dtype", f(KP, lengths=np.zeros(16))
    yield fx, "lengths_shape", f(KP, lengths=f32(15))
    yield fx, "lengths_tracks", f([KP, KP], lengths=f32(3, 16))
    yield fx, "lengths_empty_list", f([], lengths=f32(2, 16))
    yield fx, "lengths_meta", f(KP, lengths=torch.zeros(16, device="meta"))
    yield fx, "lengths+device", f(KP, lengths=f32(15), device="cpu")
    yield fx, "lengths_dtype+device", f(KP, lengths=np.zeros(16), device="cpu")
    yield fx, "device_with_lengths", f(KP, lengths=f32(16), device="cpu")
    yield fx, "device_empty_list", f([], return_lengths=True, device="cpu")


def cases():
    out = [c for gen in (_lift_cases, _stream_cases, _tracked_cases, _smooth_cases, _bones_cases) for c in gen()]
    ids = [(call, case) for call, case, _ in out]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    return out


def raise_lines():
    """Every raise statement of MODULES (those that exist): ``(module, line, source text)``."""
    out = []
    for m in MODULES:
        path = os.path.join(ROOT, "kasportsformer_amd", m)
        if os.path.exists(path):
            src = open(path).read()
            out += [(m, n.lineno, ast.get_source_segment(src, n)) for n in ast.walk(ast.parse(src)) if isinstance(n, ast.Raise)]
    return sorted(out)


def replay(lines=None):
    """Makes every call of the table -> one record per case: the call, the case id, the exception's class name and its text.  Every call must be refused, with
    a message that begins with the call's name.  With ``lines`` (a set), the (file name, line) pairs of MODULES executed on the way are added to it."""
    files = {os.path.join(ROOT, "kasportsformer_amd", m) for m in MODULES}

    def local(frame, event, arg):
        if event == "line":
            lines.add((os.path.basename(frame.f_code.co_filename), frame.f_lineno))
        return local

    def tracer(frame, event, arg):
        return local if frame.f_code.co_filename in files else None
    records = []
    for call, case, thunk in cases():
        if lines is not None:
            sys.settrace(tracer)
        try:
            thunk()
        except Exception as e:                                       # noqa: BLE001 -- the class is part of the record
            sys.settrace(None)
            assert str(e).startswith(call + ":") or str(e).startswith(call + " "), f"{call} / {case}: not a refusal of the call's own: {type(e).__name__}: {e}"
            records.append({"call": call, "case": case, "type": type(e).__name__, "message": str(e)})
        else:
            sys.settrace(None)
            raise AssertionError(f"{call} / {case}: was not refused")
    return records
