"""``python -m kasportsformer_amd.lift``: what the command line refuses about --refine and --refine-poses, and what it fills in, before anything is loaded."""
import pytest

from kasportsformer_amd.lift import _parse

BASE = ["--config", "c.yaml", "--checkpoint", "c.pth", "--keypoints", "k.npy", "--width", "1280", "--height", "720", "--out", "o.npy"]


@pytest.mark.parametrize("extra,text", [
    (["--refine", "--smooth"], "--refine and --smooth both clean up the keypoints"),
    (["--refine-min-score", "0.2"], "belong to --refine"),
    (["--refine-max-gap", "4"], "belong to --refine"),
    (["--refine-sigma", "1.5"], "belong to --refine"),
    (["--refine-poses", "--refine-sigma", "1.5"], "belong to --refine"),
    (["--refine", "--online"], "they need the frames after"),
    (["--refine-poses", "--online"], "they need the frames after"),
    (["--refine", "--refine-max-gap", "a"], "invalid int value"),
])
def test_refused_combinations(extra, text, capsys):
    with pytest.raises(SystemExit) as e:
        _parse(BASE + extra)
    assert e.value.code == 2
    assert text in capsys.readouterr().err


def test_defaults_and_values():
    a = _parse(BASE)
    assert not a.refine and not a.refine_poses
    a = _parse(BASE + ["--refine"])
    assert a.refine and (a.refine_min_score, a.refine_max_gap, a.refine_sigma) == (0.3, 15, 2.0) and not a.smooth
    a = _parse(BASE + ["--refine", "--refine-min-score", "0.5", "--refine-max-gap", "0", "--refine-sigma", "3", "--refine-poses", "--fix-bones", "--world"])
    assert (a.refine_min_score, a.refine_max_gap, a.refine_sigma) == (0.5, 0, 3.0) and a.refine_poses and a.fix_bones
    a = _parse(BASE + ["--smooth", "--refine-poses"])                              # the causal filter in front, the zero-phase one behind the lift
    assert a.smooth and a.refine_poses and not a.refine
    a = _parse(BASE + ["--smooth", "--online"])                                    # what was allowed stays allowed
    assert a.smooth and a.online
