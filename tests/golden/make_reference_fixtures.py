"""Writes the two fixtures that carry what the tests need of a Radiative3D checkout, so that the
tests themselves run without one (nothing of the reference's sources goes into the repository):

  reference_do_scripts.json   the argument list each do-script hands to ./main, captured by running
                              the script as it lies in the checkout from a scratch directory that
                              holds symbolic links to the scripts, `scripts/` and `vis/`, a Makefile
                              for which `make -q` succeeds (scripts/do-fundamentals.sh:145-152) and a
                              stand-in ./main that writes its arguments to a file
                              (tests/test_do_scripts.py)
  reference_user_models.json  for each model of tests/test_user_models_compile.py: the reference's
                              user.cpp + user_*_inc.cpp compiled against this repository's grid.hpp
                              and host builder, and the SHA-256 of the grid dump and of the cell table
                              they produce, with the cell and scatterer counts and the cell kind

    python tests/golden/make_reference_fixtures.py <Radiative3D checkout>
"""
import ctypes as C
import glob
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from radiative3d_amd import _ffi                                      # noqa: E402
from tests.configs import CONFIGS                                     # noqa: E402
from tests.test_do_scripts import CASES, case_id                      # noqa: E402
from tests.test_user_models_compile import EXTRA, MODELS, selector_args, SELECTORS  # noqa: E402

HOST = os.path.join(REPO, "radiative3d_amd", "host")


def run_do_script(ref, work, script, edit=None):
    """Run do-script `script` of checkout `ref` in scratch directory `work`; returns the tokens ./main was given."""
    os.makedirs(work)
    for entry in os.listdir(ref):
        if entry.startswith("do-") and entry.endswith(".sh"):
            os.symlink(os.path.join(ref, entry), os.path.join(work, entry))
    os.symlink(os.path.join(ref, "scripts"), os.path.join(work, "scripts"))
    os.symlink(os.path.join(ref, "vis"), os.path.join(work, "vis"))
    if edit:   # a user's one-line choice inside the script (the scripts say "copy and edit this file")
        text = open(os.path.join(ref, script)).read()
        assert edit[0] in text
        os.unlink(os.path.join(work, script))
        open(os.path.join(work, script), "w").write(text.replace(edit[0], edit[1], 1))
    argv_file = os.path.join(work, "argv.txt")
    main = os.path.join(work, "main")
    open(main, "w").write('#!/bin/bash\nprintf \'%s\\n\' "$@" > "$R3D_ARGV_OUT"\n'
                          'echo "#  R3D_GRID:"; echo "#  END R3D_GRID"\n')
    os.chmod(main, 0o755)
    open(os.path.join(work, "Makefile"), "w").write("main:\n")
    assert subprocess.run(["make", "-q"], cwd=work).returncode == 0
    env = dict(os.environ, R3D_ARGV_OUT=argv_file)
    # (figure generation follows the run and needs octave: its errors are not what is captured)
    subprocess.run(["bash", "./" + script, "noseis"], cwd=work, env=env, capture_output=True, text=True, timeout=120)
    assert os.path.exists(argv_file), f"{script} never reached ./main"
    return open(argv_file).read().split("\n")[:-1]


def user_lib(ref, tmp):
    out = os.path.join(tmp, "libr3d_host_user.so")
    srcs = [f for f in glob.glob(os.path.join(HOST, "*.cpp")) if os.path.basename(f) not in ("main.cpp", "scatter_out.cpp", "batch_out.cpp")]   # (the three of ./main)
    # user.cpp says #include "grid.hpp": feed it on stdin so that the quote-include resolves through -I to
    # THIS repository's grid.hpp, and the user_*_inc.cpp files through the second -I to the checkout
    cmd = ["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-pthread", "-I", HOST, "-I", ref,
           "-o", out, "-x", "c++", "-", "-x", "none"] + srcs
    with open(os.path.join(ref, "user.cpp")) as f:
        subprocess.check_call(cmd, stdin=f, cwd=tmp)
    L = C.CDLL(out)
    L.r3dh_model_from_args.restype = C.c_void_p
    L.r3dh_model_from_args.argtypes = [C.c_int, C.POINTER(C.c_char_p)]
    L.r3dh_model_desc.restype = C.POINTER(_ffi.ModelDesc)
    L.r3dh_model_desc.argtypes = [C.c_void_p]
    L.r3dh_grid_dump.restype = C.c_char_p
    L.r3dh_grid_dump.argtypes = [C.c_void_p]
    L.r3dh_model_free.argtypes = [C.c_void_p]
    L.r3dh_last_error.restype = C.c_char_p
    return L


def digest(lib, args):
    argv = (C.c_char_p * len(args))(*[a.encode() for a in args])
    h = lib.r3dh_model_from_args(len(args), argv)
    assert h, lib.r3dh_last_error().decode()
    d = lib.r3dh_model_desc(h).contents
    cells = C.string_at(d.cells, C.sizeof(_ffi.Cell) * d.n_cells)
    rec = {"args": list(args), "grid_dump_sha256": hashlib.sha256(lib.r3dh_grid_dump(h)).hexdigest(),
           "cells_sha256": hashlib.sha256(cells).hexdigest(), "n_cells": d.n_cells,
           "n_scatterers": d.n_scatterers, "cell_kind": d.cell_kind}
    lib.r3dh_model_free(h)
    return rec


def main(ref):
    ref = os.path.abspath(ref)
    tmp = tempfile.mkdtemp()
    try:
        scripts = {}
        for script, edit, _ in CASES:
            scripts[case_id(script, edit)] = {"script": script, "edit": list(edit) if edit else None,
                                              "argv": run_do_script(ref, os.path.join(tmp, case_id(script, edit)),
                                                                    script, edit)}
        json.dump({"_provenance": "argument lists the do-scripts of an unmodified Radiative3D checkout hand to "
                                  "./main (run with the argument `noseis`); tests/golden/make_reference_fixtures.py",
                   "scripts": scripts},
                  open(os.path.join(HERE, "reference_do_scripts.json"), "w"), indent=1)
        L = user_lib(ref, tmp)
        models = {name: digest(L, EXTRA[name] if name in EXTRA else CONFIGS[name](2)) for name in MODELS}
        selectors = {str(sel): digest(L, selector_args(sel)) for sel in SELECTORS}
        json.dump({"_provenance": "an unmodified Radiative3D checkout's user.cpp + user_*_inc.cpp compiled against "
                                  "this repository's grid.hpp and host builder: SHA-256 of r3dh_grid_dump and of the "
                                  "r3d_cell table of each model; tests/golden/make_reference_fixtures.py",
                   "models": models, "selectors": selectors},
                  open(os.path.join(HERE, "reference_user_models.json"), "w"), indent=1)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
