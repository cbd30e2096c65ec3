"""./main for the tests, and the scatter-grid job that the CLI tests of the views and of the maps both run."""
import os
import subprocess

from radiative3d_amd import _ffi
from radiative3d_amd.model import volume_desc
from tests.configs import crustpinch

GRID_OPT = "--scatter-grid=64,60,14,35,-200,-600,-130,1080,600,10"
GRID_ARGS = crustpinch(4) + ["--overridemfp=25,50", "--nodeflect", "--timetolive=350", "--num-phonons=20K", GRID_OPT]


def main_exe():
    exe = os.path.join(_ffi.REPO, "main")
    assert os.path.exists(exe), "./main was not built"
    return exe


def grid_desc():
    """GRID_OPT over the job's 350 s, as the engine sees it."""
    return volume_desc((-200.0, -600.0, -130.0), (20.0, 20.0, 10.0), (64, 60, 14), 35, 10.0)


def run(tmp_path, name, extra):
    """./main GRID_ARGS + extra in a new directory tmp_path/name: that directory, the names of its files, stdout."""
    out = tmp_path / name
    out.mkdir()
    r = subprocess.run([main_exe()] + GRID_ARGS + extra + [f"--output-dir={out}"], cwd=out, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    files = set(os.listdir(out))
    assert not [f for f in files if f.endswith(".part")]
    return out, files, r.stdout
