"""Shared by tests/test_gpu_lift.py, test_gpu_lift_tracks.py, test_gpu_stream.py and tests/test_lift_host_cpu.py (not a test): numpy / torch restatements of
the demo's arithmetic (demo/demo.py:132-156,222-236, demo/lib/utils.py:5-20) that the lifting kernels are held to bit for bit -- the windows of a track cut,
normalised and mirrored, the flip-TTA merge stitched back on the track, and the same for the current window of a stream slot."""
import numpy as np
import torch

LEFT, RIGHT = [1, 2, 3, 14, 15, 16], [4, 5, 6, 11, 12, 13]
W_PX, H_PX = 1280, 720


def _flip_np(a):
    """flip_data (demo/lib/utils.py:5-13) on a copy."""
    f = a.copy()
    f[..., 0] *= -1
    f[..., LEFT + RIGHT, :] = f[..., RIGHT + LEFT, :]
    return f


def _flip_t(a):
    f = a.clone()
    f[..., 0] *= -1
    f[..., LEFT + RIGHT, :] = f[..., RIGHT + LEFT, :]
    return f


def _track(P, N, seed):
    g = np.random.default_rng(seed)
    xy = g.uniform((0, 0), (W_PX, H_PX), size=(P, N, 17, 2))
    return np.concatenate((xy, g.uniform(0.2, 1.0, size=(P, N, 17, 1))), axis=-1).astype(np.float32)


def _windows_np(kp, T, s, flip):
    """The demo's clips (or the overlap plan) of every person, normalised with normalize_screen_coordinates's own expression."""
    from kasportsformer_amd.lift import window_plan
    starts, lengths, r, _ = window_plan(kp.shape[1], T, s)
    clips = []
    for p in range(kp.shape[0]):
        for a, L in zip(starts, lengths):
            c = kp[p, a:a + L]
            if L < T:
                c = c[r]
            res = np.copy(c)
            res[..., :2] = c[..., :2] / W_PX * 2 - [1, H_PX / W_PX]
            clips.append(res)
    x = np.stack(clips)
    return np.concatenate((x, _flip_np(x))) if flip else x


def _stitch_t(pred, P, N, T, s, flip):
    """(p + flip(p_f)) / 2, root zeroed, per window; frames of a resampled window read first_pos; covering windows summed in ascending order, then divided."""
    from kasportsformer_amd.lift import window_plan
    starts, lengths, _, fp = window_plan(N, T, s)
    W = len(starts)
    merged = (pred[:P * W] + _flip_t(pred[P * W:])) / 2 if flip else pred[:P * W].clone()
    merged[:, :, 0, :] = 0
    merged = merged.view(P, W, T, 17, 3)
    acc = torch.zeros(P, N, 17, 3)
    cnt = torch.zeros(N)
    for w, (a, L) in enumerate(zip(starts, lengths)):
        win = merged[:, w, torch.from_numpy(fp).long()] if L < T else merged[:, w]
        acc[:, a:a + L] += win
        cnt[a:a + L] += 1
    return acc / cnt.view(1, N, 1, 1)


def _frames(n, seed):
    return _track(1, n, seed=seed)[0]                                   # [n,17,3] pixels + confidence


def _clip_np(w, T, w_px, h_px):
    """test_gpu_lift._windows_np's expression on one window of L <= T frames (L < T: the demo's resampled clip), normalised at w_px x h_px."""
    from kasportsformer_amd.lift import window_plan
    r = window_plan(w.shape[0], T)[2]
    c = w[r] if r is not None else w
    res = np.copy(c)
    res[..., :2] = c[..., :2] / w_px * 2 - [1, h_px / w_px]
    return res


def _windows_stream_np(windows, T, res, flip):
    """Clip h * K + i: window i of the call, mirrored when h == 1."""
    x = np.stack([_clip_np(w, T, *wh) for w, wh in zip(windows, res)])
    return np.concatenate((x, _flip_np(x))) if flip else x


def _emit_t(pred, Ls, T, back, n_out, flip):
    """test_gpu_lift._stitch_t on each slot's one window (plain and mirrored clip), then rows clamp(L - 1 - back + r, 0, L - 1)."""
    K = len(Ls)
    rows = []
    for i, L in enumerate(Ls):
        mine = torch.cat((pred[i:i + 1], pred[K + i:K + i + 1])) if flip else pred[i:i + 1]
        st = _stitch_t(mine, 1, L, T, T, flip)[0]
        rows.append(st[[min(max(L - 1 - back + r, 0), L - 1) for r in range(n_out)]])
    return torch.stack(rows)


def _ring_state(T, ks, seed):
    """Histories of ks[s] frames per slot and the ring / count they leave: frame number c at ring position c % T; unwritten positions hold -1."""
    hist = [_frames(k, seed + 5 * s) for s, k in enumerate(ks)]
    ring = np.full((len(ks), T, 17, 3), -1.0, np.float32)
    for s, h in enumerate(hist):
        for c in range(len(h)):
            ring[s, c % T] = h[c]
    return hist, ring, np.asarray(ks, np.int64)
