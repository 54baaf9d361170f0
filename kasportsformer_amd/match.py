"""Matching players across cameras: which of the rows that C calibrated cameras' trackers emit are the same player, on the device.

    cams = np.stack([camera_row((fx, fy, cx, cy), (k1, k2, p1, p2, k3), R, t) for ...])   # [C,21]; X_cam = R X_world + t, a static rig
    m = match_players([kp_cam0, kp_cam1, ...], cams)                # each [P_c,N,J,3] pixel x, pixel y, score: a camera's P_c tracked rows over N frames
    m.group, m.members, m.views, m.group_cost, m.count, m.dropped   # [C,P], [G,C], [G] int32, [G] float32, two int32 scalars -- all on the device
    joints = triangulate_keypoints(gather_matched(kp, m), cams).points                       # [G,N,J,3] in the world frame, nothing read back
    c = match_costs(kp, cams); g = match_groups(c.cost, c.samples)  # the two stages on their own

include/kasf.h (``kasf_match_pair_costs``, ``kasf_match_groups``) states both rules in full, once.  The cost of a pair of rows of two cameras is the mean,
over the joints and frames at which both keypoints are usable, of the gap between the two undistorted rays at their closest approach, in pixels at the two
depths, capped at ``cap`` and weighted by the product of the scores; fewer than ``min_samples`` comparable samples give +inf.  The grouping takes the cameras
in ascending order: a camera's rows are assigned to the existing groups by the optimal assignment of the sample-weighted mean cost to each group's members, a
pair above ``max_cost`` is rejected, and the rows left over open new groups.  So the result depends on the order of the cameras -- the first camera's rows
seed the groups -- which is a property of the rule.  Every sum runs in a fixed order: the same bits from run to run, and a pair's cost does not depend on
which other cameras are given.  Three launches, nothing read back, no host path.

Not here: synchronising the cameras in time (frame n is the same instant in every camera), moving cameras (``cameras`` is one row per camera), a stateful
live matcher that keeps group ids from tick to tick (a live tick is a call with N = 1 and starts from nothing), and cycle-consistent multi-way matching.  The
defaults -- ``cap`` 50 px, ``max_cost`` 15 px, ``min_samples`` 2 J -- are a starting point, not tuned: nothing was run on footage.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np
import torch

from . import _args, _lib
from ._args import index_in, number
from .triangulate import CAMERA_FLOATS, MAX_ROUNDS

MIN_CAMERAS, MAX_CAMERAS, MAX_ROWS = 2, _lib.MATCH_MAX_CAMERAS, _lib.MATCH_MAX_ROWS


class MatchCosts(NamedTuple):
    """What ``match_costs`` returns, on the device: ``cost`` [C,C,P,P] float32 (pixels; +inf where fewer than ``min_samples`` samples were comparable and in
    the diagonal blocks; ``cost[b,a,q,p]`` has the bits of ``cost[a,b,p,q]``) and ``samples`` [C,C,P,P] int32, the comparable samples of each pair."""
    cost: torch.Tensor
    samples: torch.Tensor


class MatchGroups(NamedTuple):
    """What ``match_groups`` returns, on the device: ``group`` [C,P] int32 (a row's group, -1 for an empty or a dropped row), ``members`` [G,C] int32 (a
    group's row in each camera, -1 for none), ``views`` [G] int32, ``group_cost`` [G] float32 (the mean cost at which its rows were accepted, NaN for a group of
    one view), ``count`` and ``dropped``: int32 scalars."""
    group: torch.Tensor
    members: torch.Tensor
    views: torch.Tensor
    group_cost: torch.Tensor
    count: torch.Tensor
    dropped: torch.Tensor


class MatchResult(NamedTuple):
    """What ``match_players`` returns: the fields of ``MatchGroups`` and of ``MatchCosts``, all on the device."""
    group: torch.Tensor
    members: torch.Tensor
    views: torch.Tensor
    group_cost: torch.Tensor
    count: torch.Tensor
    dropped: torch.Tensor
    cost: torch.Tensor
    samples: torch.Tensor


def match_params(joints: int, min_score=0.3, weighted=True, cap=50.0, min_samples=None, undistort_iterations=5, who: str = "match_costs") -> _lib.KasfMatchParams:
    """The parameters as the entry point takes them, refused as the entry point refuses them; ``min_samples`` None: 2 * joints."""
    min_score, cap = number(min_score, who, "min_score"), number(cap, who, "cap")
    if not np.float32(cap) > 0:
        raise ValueError(f"{who}: cap must be > 0 pixels, got {cap}")
    if not isinstance(weighted, (bool, np.bool_)):
        raise TypeError(f"{who}: weighted must be a bool, got {type(weighted).__name__}")
    min_samples = 2 * joints if min_samples is None else index_in(min_samples, who, "min_samples", 1, 2 ** 31 - 1)
    undistort_iterations = index_in(undistort_iterations, who, "undistort_iterations", 0, MAX_ROUNDS)
    return _lib.KasfMatchParams(min_score, int(weighted), cap, min_samples, undistort_iterations)


def _group_params(max_cost, max_groups, rows: int, who: str):
    max_cost = number(max_cost, who, "max_cost")
    if not np.float32(max_cost) > 0:
        raise ValueError(f"{who}: max_cost must be > 0 pixels, got {max_cost}")
    return max_cost, (min(MAX_ROWS, 2 * rows) if max_groups is None else index_in(max_groups, who, "max_groups", 1, MAX_ROWS))


def _tracks(keypoints, who: str):
    """keypoints [C,P,N,J,3], or a list of C arrays [P_c,N,J,3] -> (the tensors where they are, the shape (C, P, N, J) of the padded whole)."""
    if isinstance(keypoints, (list, tuple)):
        parts = [_args.as_tensor(a, who, f"keypoints[{i}]", _args.FLOAT32) for i, a in enumerate(keypoints)]
        if not MIN_CAMERAS <= len(parts) <= MAX_CAMERAS:
            raise ValueError(f"{who}: expected the keypoints of 2 to 16 cameras, got {len(parts)}")
        if any(p.dim() != 4 or p.shape[-1] != 3 or p.shape[-2] < 1 for p in parts):
            raise ValueError(f"{who}: expected every camera's keypoints as [P,N,J,3] with J >= 1, got {[tuple(p.shape) for p in parts]}")
        if any(tuple(p.shape[1:]) != tuple(parts[0].shape[1:]) for p in parts):
            raise ValueError(f"{who}: every camera's keypoints must have one N and one J, got {[tuple(p.shape) for p in parts]}")
        shape = (len(parts), max(int(p.shape[0]) for p in parts)) + tuple(int(v) for v in parts[0].shape[1:3])
    else:
        parts = [_args.as_tensor(keypoints, who, "keypoints", _args.FLOAT32)]
        k = parts[0]
        if k.dim() != 5 or k.shape[-1] != 3 or k.shape[-2] < 1:
            raise ValueError(f"{who}: expected keypoints of [C,P,N,J,3] with J >= 1, or a list of C arrays [P,N,J,3], got {tuple(k.shape)}")
        if not MIN_CAMERAS <= k.shape[0] <= MAX_CAMERAS:
            raise ValueError(f"{who}: expected the keypoints of 2 to 16 cameras, got {k.shape[0]}")
        shape = tuple(int(v) for v in k.shape[:4])
    if not 1 <= shape[1] <= MAX_ROWS:
        raise ValueError(f"{who}: expected 1 to 64 rows per camera, got {shape[1]}")
    if shape[2] * shape[3] >= 2 ** 31:
        raise ValueError(f"{who}: N * J must stay below 2^31, got {shape[2]} * {shape[3]}")
    return parts, shape, isinstance(keypoints, (list, tuple))


def _on_device(parts, shape, listed: bool, dev) -> torch.Tensor:
    """The padded whole [C,P,N,J,3] on the device: a camera with fewer rows is filled up with rows of score 0."""
    if not listed:
        return parts[0].to(dev).contiguous()
    k = torch.zeros(shape + (3,), dtype=torch.float32, device=dev)
    for c, p in enumerate(parts):
        k[c, :p.shape[0]] = p.to(dev)
    return k


def _cameras(cameras, views: int, who: str) -> torch.Tensor:
    cam = _args.as_tensor(cameras, who, "cameras", _args.FLOAT32)
    if tuple(cam.shape) != (views, CAMERA_FLOATS):
        raise ValueError(f"{who}: cameras must be [{views}, 21] (fx, fy, cx, cy, k1, k2, p1, p2, k3, R, t), one row per camera of a static rig, got "
                         f"{tuple(cam.shape)}")
    return cam


def _pair_costs(k: torch.Tensor, cam: torch.Tensor, params, dev) -> MatchCosts:
    views, rows, N, J = (int(v) for v in k.shape[:4])
    if N == 0:                                                          # nothing to compare: no launch
        return MatchCosts(torch.full((views, views, rows, rows), float("inf"), dtype=torch.float32, device=dev),
                          torch.zeros((views, views, rows, rows), dtype=torch.int32, device=dev))
    cost = torch.empty((views, views, rows, rows), dtype=torch.float32, device=dev)
    samples = torch.empty((views, views, rows, rows), dtype=torch.int32, device=dev)
    lib = _lib.load()
    nbytes = int(lib.kasf_match_workspace_bytes(views, rows, N))
    if nbytes < 0:
        _lib.check(int(-nbytes))
    work = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.kasf_match_pair_costs(k.data_ptr(), views, rows, N, J, cam.data_ptr(), C.byref(params), cost.data_ptr(), samples.data_ptr(),
                                             work.data_ptr(), nbytes, _args.stream()))
    return MatchCosts(cost, samples)


def _groups(cost: torch.Tensor, samples: torch.Tensor, max_cost: float, G: int, dev) -> MatchGroups:
    views, rows = int(cost.shape[0]), int(cost.shape[2])
    group = torch.empty((views, rows), dtype=torch.int32, device=dev)
    members = torch.empty((G, views), dtype=torch.int32, device=dev)
    n_views, group_cost = torch.empty(G, dtype=torch.int32, device=dev), torch.empty(G, dtype=torch.float32, device=dev)
    count, dropped = torch.empty((), dtype=torch.int32, device=dev), torch.empty((), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().kasf_match_groups(cost.data_ptr(), samples.data_ptr(), views, rows, max_cost, G, group.data_ptr(), members.data_ptr(),
                                                 n_views.data_ptr(), group_cost.data_ptr(), count.data_ptr(), dropped.data_ptr(), _args.stream()))
    return MatchGroups(group, members, n_views, group_cost, count, dropped)


def match_costs(keypoints, cameras, *, min_score: float = 0.3, weighted: bool = True, cap: float = 50.0, min_samples=None, undistort_iterations: int = 5,
                device=None) -> MatchCosts:
    """The cost of every pair of rows of two cameras; see the module docstring.  ``keypoints``: [C,P,N,J,3] (pixel x, pixel y, score), or a list of C arrays
    [P_c,N,J,3] whose P_c may differ (a camera with fewer rows is padded on the device with rows of score 0), 2 <= C <= 16, 1 <= P <= 64: float32, numpy or
    torch, on the host or the GPU, never modified.  ``cameras``: float32 [C,21] (``camera_row``).  ``min_score``: a keypoint scored below it is not used;
    ``weighted``: weigh a sample by the product of its two scores; ``cap`` > 0 pixels: what one sample can cost at most; ``min_samples`` >= 1 (default 2 J):
    a pair with fewer comparable samples costs +inf; ``undistort_iterations`` in [0, 20].  -> ``MatchCosts`` on the device.  Two launches, none with N = 0.
    Every refusal is raised before any launch."""
    who = "match_costs"
    parts, shape, listed = _tracks(keypoints, who)
    params = match_params(shape[3], min_score, weighted, cap, min_samples, undistort_iterations, who)
    cam = _cameras(cameras, shape[0], who)
    dev = _args.resolve_device(parts + [cam], device, who)
    return _pair_costs(_on_device(parts, shape, listed, dev), cam.to(dev).contiguous(), params, dev)


def match_groups(cost, samples, *, max_cost: float = 15.0, max_groups=None, device=None) -> MatchGroups:
    """Groups of rows, one row per camera at most, from any ``cost`` float32 and ``samples`` int32 [C,C,P,P] (``match_costs`` gives them; so may anything else).
    ``max_cost`` > 0 pixels: a row joins a group at this cost at most; ``max_groups`` G in [1, 64] (default min(64, 2 P)): rows that would open a group beyond
    it are counted in ``dropped``.  -> ``MatchGroups`` on the device.  One launch.  Every refusal is raised before any launch."""
    who = "match_groups"
    c = _args.as_tensor(cost, who, "cost", _args.FLOAT32)
    if isinstance(samples, np.ndarray) and samples.dtype == np.int32:   # _args.as_tensor knows no integer numpy type
        s = torch.from_numpy(np.ascontiguousarray(samples))
    else:
        s = _args.as_tensor(samples, who, "samples", (torch.int32,))
    if c.dim() != 4 or c.shape[0] != c.shape[1] or c.shape[2] != c.shape[3] or not MIN_CAMERAS <= c.shape[0] <= MAX_CAMERAS or not 1 <= c.shape[2] <= MAX_ROWS:
        raise ValueError(f"{who}: expected cost of [C,C,P,P] with 2 <= C <= 16 and 1 <= P <= 64, got {tuple(c.shape)}")
    if tuple(s.shape) != tuple(c.shape):
        raise ValueError(f"{who}: samples must have the shape of cost, {tuple(c.shape)}, got {tuple(s.shape)}")
    max_cost, G = _group_params(max_cost, max_groups, int(c.shape[2]), who)
    dev = _args.resolve_device([c, s], device, who)
    return _groups(c.to(dev).contiguous(), s.to(dev).contiguous(), max_cost, G, dev)


def match_players(keypoints, cameras, *, min_score: float = 0.3, weighted: bool = True, cap: float = 50.0, min_samples=None, undistort_iterations: int = 5,
                  max_cost: float = 15.0, max_groups=None, device=None) -> MatchResult:
    """``match_costs`` and ``match_groups`` in one call, with their arguments: three launches on the current stream, no synchronisation, nothing read back.
    -> ``MatchResult`` on the device."""
    who = "match_players"
    parts, shape, listed = _tracks(keypoints, who)
    params = match_params(shape[3], min_score, weighted, cap, min_samples, undistort_iterations, who)
    max_cost, G = _group_params(max_cost, max_groups, shape[1], who)
    cam = _cameras(cameras, shape[0], who)
    dev = _args.resolve_device(parts + [cam], device, who)
    costs = _pair_costs(_on_device(parts, shape, listed, dev), cam.to(dev).contiguous(), params, dev)
    return MatchResult(*_groups(costs.cost, costs.samples, max_cost, G, dev), costs.cost, costs.samples)


def gather_matched(keypoints, match, *, device=None) -> torch.Tensor:
    """The tracks in group order: ``keypoints`` as ``match_players`` took them and its result (or a ``MatchGroups``) -> float32 [C,G,N,J,3] on the device; row
    g of camera c is group g's track there, and zero -- coordinates and score -- where the group has no member in that camera, so that
    ``triangulate_keypoints(gather_matched(kp, m), cams).points`` is [G,N,J,3].  Indexing on the device, nothing read back."""
    who = "gather_matched"
    parts, shape, listed = _tracks(keypoints, who)
    members = getattr(match, "members", None)
    if not isinstance(members, torch.Tensor) or members.dtype != torch.int32 or members.dim() != 2 or members.shape[1] != shape[0]:
        raise ValueError(f"{who}: match must be the result of match_players or match_groups for these {shape[0]} cameras")
    dev = _args.resolve_device(parts + [members], device, who)
    k = _on_device(parts, shape, listed, dev)
    row = members.to(dev).t().long()                                    # [C,G]
    out = k[torch.arange(shape[0], device=dev)[:, None], row.clamp(min=0)]
    return torch.where((row >= 0)[:, :, None, None, None], out, torch.zeros((), dtype=torch.float32, device=dev))
