"""``python -m kasportsformer_amd.lift``: what the command line refuses about --place, and what it fills in, before anything is loaded."""
import numpy as np
import pytest

from kasportsformer_amd.lift import _parse, main

BASE = ["--config", "c.yaml", "--checkpoint", "c.pth", "--keypoints", "k.npy", "--width", "1280", "--height", "720", "--out", "o.npy"]
CAM = ["--camera", "1500,1500,960,540"]


@pytest.mark.parametrize("extra,text", [
    (["--place"], "--place needs --camera FX,FY,CX,CY"),
    (CAM, "belong to --place"),
    (["--place-lengths", "t.npy"], "belong to --place"),
    (["--place-iterations", "2"], "belong to --place"),
    (["--place-delta", "2.0"], "belong to --place"),
    (["--place", *CAM, "--world", "--world-unit"], "--place is refused with --world-unit"),
    (["--place", "--camera", "1500,1500,960"], "--camera must be four finite numbers"),
    (["--place", "--camera", "1500,1500,960,540,1"], "--camera must be four finite numbers"),
    (["--place", "--camera", "1500,x,960,540"], "--camera must be four finite numbers"),
    (["--place", "--camera", "1500,nan,960,540"], "--camera must be four finite numbers"),
    (["--place", "--camera", "0,1500,960,540"], "--camera must be four finite numbers"),
    (["--place", "--camera=-1500,1500,960,540"], "--camera must be four finite numbers"),
    (["--place", *CAM, "--place-iterations", "9"], "--place-iterations must be in [0, 8]"),
    (["--place", *CAM, "--place-iterations", "-1"], "--place-iterations must be in [0, 8]"),
    (["--place", *CAM, "--place-iterations", "a"], "invalid int value"),
    (["--place", *CAM, "--place-delta", "0"], "--place-delta must be finite and > 0"),
    (["--place", *CAM, "--place-delta", "nan"], "--place-delta must be finite and > 0"),
])
def test_refused_combinations(extra, text, capsys):
    with pytest.raises(SystemExit) as e:
        _parse(BASE + extra)
    assert e.value.code == 2
    assert text in capsys.readouterr().err


def test_defaults_and_values():
    a = _parse(BASE)
    assert not a.place and a.camera is None and a.place_lengths is None
    a = _parse(BASE + ["--place", *CAM])
    assert a.place and a.camera.dtype == np.float32 and a.camera.tolist() == [1500.0, 1500.0, 960.0, 540.0]
    assert (a.place_iterations, a.place_delta, a.place_lengths) == (4, 3.0, None)
    a = _parse(BASE + ["--place", "--camera", "1400.5,1390,955.25,541", "--place-iterations", "0", "--place-delta", "1.5", "--place-lengths", "t.npy",
                       "--refine-poses", "--fix-bones", "--world", "--world-floor"])
    assert (a.place_iterations, a.place_delta, a.place_lengths) == (0, 1.5, "t.npy") and a.world_floor and a.fix_bones and a.refine_poses
    a = _parse(BASE + ["--place", *CAM, "--online"])                               # frames are independent: the live replay can be placed too
    assert a.place and a.online


def test_a_bad_bone_table_is_refused_before_the_model_is_loaded(tmp_path):
    """The config does not exist: a run that got as far as loading it would raise FileNotFoundError for c.yaml, not the table's error."""
    np.save(tmp_path / "t.npy", np.zeros(16))
    with pytest.raises(ValueError, match="the bone lengths must be finite"):
        main(BASE + ["--place", *CAM, "--place-lengths", str(tmp_path / "t.npy")])
    with pytest.raises(FileNotFoundError, match="missing.npy"):
        main(BASE + ["--place", *CAM, "--place-lengths", str(tmp_path / "missing.npy")])
