"""``python -m kasportsformer_amd.lift``: what the command line refuses about --camera-distortion, and what it fills in, before anything is loaded."""
import numpy as np
import pytest

from kasportsformer_amd.lift import _parse

BASE = ["--config", "c.yaml", "--checkpoint", "c.pth", "--keypoints", "k.npy", "--width", "1280", "--height", "720", "--out", "o.npy"]
PLACE = ["--place", "--camera", "1500,1500,960,540"]
FIVE = "--camera-distortion must be five finite numbers K1,K2,P1,P2,K3"


@pytest.mark.parametrize("extra,text", [
    (["--camera-distortion=-0.12,0.05,0,0,0"], "--camera-distortion belongs to --place"),
    (["--camera", "1500,1500,960,540", "--camera-distortion=-0.12,0.05,0,0,0"], "belong to --place"),
    ([*PLACE, "--camera-distortion=-0.12,0.05,0,0"], FIVE),
    ([*PLACE, "--camera-distortion=-0.12,0.05,0,0,0,0"], FIVE),
    ([*PLACE, "--camera-distortion", ""], FIVE),
    ([*PLACE, "--camera-distortion=-0.12,x,0,0,0"], FIVE),
    ([*PLACE, "--camera-distortion=-0.12,nan,0,0,0"], FIVE),
    ([*PLACE, "--camera-distortion=-0.12,0.05,0,0,inf"], FIVE),
    ([*PLACE, "--camera-distortion=-0.12,0.05,0,0,1e39"], FIVE),            # not finite as the float32 the device takes
    ([*PLACE, "--camera-distortion"], "expected one argument"),
])
def test_refused_combinations(extra, text, capsys):
    with pytest.raises(SystemExit) as e:
        _parse(BASE + extra)
    assert e.value.code == 2
    assert text in capsys.readouterr().err


def test_defaults_and_values():
    assert _parse(BASE).camera_distortion is None
    assert _parse(BASE + PLACE).camera_distortion is None                       # without the flag nothing changes
    a = _parse(BASE + PLACE + ["--camera-distortion=-0.12,0.05,0.001,-0.0005,0.01"])
    assert a.camera_distortion.dtype == np.float32 and a.camera_distortion.tolist() == np.array([-0.12, 0.05, 0.001, -0.0005, 0.01], np.float32).tolist()
    assert a.place and a.camera.tolist() == [1500.0, 1500.0, 960.0, 540.0]
    a = _parse(BASE + PLACE + ["--camera-distortion", "0,0,0,0,0", "--online", "--layout", "coco"])
    assert a.camera_distortion.tolist() == [0.0] * 5 and a.online


def test_the_help_names_the_flag(capsys):
    with pytest.raises(SystemExit):
        _parse(["--help"])
    assert "--camera-distortion" in capsys.readouterr().out
