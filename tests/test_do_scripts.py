"""The reference's own run scripts against this repository's command line and run configurations.

north_star: "the existing do-*.sh drivers ... work unchanged".  Each do-script of an unmodified
checkout was run as it lies, from a scratch directory that held symbolic links to the scripts,
`scripts/` and `vis/`, a Makefile for which `make -q` succeeds (scripts/do-fundamentals.sh:145-152)
and a stand-in `./main` that wrote its argument list to a file; those argument lists -- what
RunSimulation assembles, scripts/do-fundamentals.sh:387-427 -- are recorded in
tests/golden/reference_do_scripts.json (written by tests/golden/make_reference_fixtures.py; nothing of
the reference's sources is copied into the repository).  They must be (a) exactly the run
configuration radiative3d_amd/configs.py transcribes and bench.py runs, at the script's TOA degree,
and (b) accepted by host/cmdline.cpp: the model builds from them."""
import json
import os
import subprocess

import pytest

from radiative3d_amd import Model, configs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_do_scripts.json")

# what a script adds for its own bookkeeping and every run shares (do-fundamentals.sh:396-419)
BOOKKEEPING = ("--reports=", "--output-dir=", "--report-file=", "--mparams-outfile=", "--num-phonons=", "--dump-grid")


def case_id(script, edit):
    return script + ("+expl" if edit else "")


def do_script_tokens(script, edit=None):
    """The tokens do-script `script` (with the one-line `edit` a user makes, if any) gave ./main."""
    rec = json.load(open(GOLDEN))["scripts"][case_id(script, edit)]
    assert (rec["script"], rec["edit"]) == (script, list(edit) if edit else None)
    return rec["argv"]


def split(tokens):
    run = [t for t in tokens if not t.startswith(BOOKKEEPING)]
    return run, [t for t in tokens if t.startswith(BOOKKEEPING)]


def toa_degree(tokens):
    return int(next(t for t in tokens if t.startswith("--toa-degree=")).split("=")[1])


CASES = [
    ("do-halfspace.sh", None, lambda d: configs.halfspace(d)),
    ("do-crustpinch.sh", None, lambda d: configs.crustpinch(d)),
    ("do-lopnor.sh", None, lambda d: configs.lopnor(d, event="eq")),
    ("do-lopnor.sh", ("event=eq ", "event=expl "), lambda d: configs.lopnor(d)),     # BASELINE config 3
    ("do-spherical.sh", None, lambda d: configs.sphere(d)),
    ("do-crustpinch-vids.sh", None, lambda d: configs.crustpinch_vids(d)),
    ("do-toysphere-vids.sh", None, lambda d: configs.toysphere_vids(d)),
    ("do-lopnor-vids.sh", None, lambda d: configs.lopnor_vids(d)),
]


@pytest.mark.parametrize("script,edit,config", CASES, ids=[case_id(c[0], c[1]) for c in CASES])
def test_do_script_tokens_are_the_run_configuration(script, edit, config):
    tokens = do_script_tokens(script, edit)
    run, book = split(tokens)
    deg = toa_degree(run)
    assert deg == (8 if "vids" in script else 9)                  # PopDefaults: waveform 9, video 8
    # (a) the transcription bench.py and the tests run: same tokens, whatever their order
    assert sorted(run) == sorted(config(deg)), (sorted(run), sorted(config(deg)))
    # every bookkeeping option the scripts pass is there once
    assert sorted(t.split("=")[0] for t in book) == sorted(b.rstrip("=") for b in BOOKKEEPING)
    # (b) host/cmdline.cpp takes the script's command line as it is (tables at a small TOA degree:
    # the option parser and the model builder are what is under test, not 5 M take-off angles)
    small = [("--toa-degree=3" if t.startswith("--toa-degree=") else t) for t in tokens
             if not t.startswith("--output-dir=")]
    m = Model(small)
    want = Model(config(3))
    assert (m.n_cells, m.n_scatterers, m.n_seismometers, m.n_bins) == (want.n_cells, want.n_scatterers,
                                                                      want.n_seismometers, want.n_bins)


def test_the_cli_accepts_a_do_script_command_line_end_to_end(tmp_path):
    """./main itself (host/main.cpp) on the tokens of do-halfspace.sh: option parsing, model build,
    grid and scatterer dumps on stdout -- up to the point where it asks for a GPU."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(repo, "main")
    if not os.path.exists(exe):
        pytest.skip("./main not built")
    tokens = do_script_tokens("do-halfspace.sh")
    out = tmp_path / "out"
    out.mkdir()
    args = [("--toa-degree=3" if t.startswith("--toa-degree=") else f"--output-dir={out}" if t.startswith("--output-dir=")
             else "--num-phonons=1K" if t.startswith("--num-phonons=") else t) for t in tokens]
    r = subprocess.run([exe] + args, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert "#  R3D_GRID:" in r.stdout and "#  END R3D_GRID" in r.stdout
    if r.returncode != 0:   # no GPU in the build container: refused with the engine's message, after the model was built
        assert "no HIP device" in r.stdout + r.stderr or "no CPU path" in r.stdout + r.stderr, r.stderr[-2000:]
