"""Writes tests/golden/cli_refusals.json: what ./main answers to command lines that combine its batched products (the
options that run with --error-batches=B, keep the run's batch blocks on one device and write one .octv file) with each
other, with --job-error-batches, with --reports and with each other's companion options.  No command line names a model:
each is refused while the options are processed, and the fixture keeps its arguments and its `** Message:` line.  Run it
against a ./main whose refusals are known to be right -- the fixture was recorded from the commit before the refusals
became one loop over a table (tests/test_cli_refusals.py replays it).

    python tests/golden/make_cli_refusals.py
"""
import itertools
import json
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# the products in the order they were introduced, each in its minimal spelling
PRODUCTS = [["--lapse-windows"], ["--ttimage"], ["--target-error=0.1,0.9,16,1"], ["--envelope-shape"], ["--envelope-fit=o"],
            ["--slant-stack=0,0.3,8"], ["--array-contrast", "--contrast-model-args=1"]]
# every companion option with one valid value
COMPANIONS = ["--lapse-axes=0,0,1", "--lapse-geospread=2", "--lapse-ranges=8,50,150", "--lapse-array=0,3",
              "--ttimage-array=0,3", "--ttimage-axes=1,1,1", "--ttimage-fit=1,3", "--ttimage-normcurve=1,-2",
              "--target-array=0,3", "--target-components=PS",
              "--envelope-array=0,3", "--envelope-axes=1,1,1",
              "--envelope-fit-array=0,3", "--envelope-fit-axes=1,1,1", "--envelope-fit-energy",
              "--slant-array=0,3", "--slant-axes=1,1,1", "--slant-energy", "--slant-range-power=1", "--slant-windows=0,10",
              "--contrast-array=0,3", "--contrast-axes=1,1,1", "--contrast-windows=4,3", "--contrast-regions=10,50",
              "--contrast-range-power=1", "--contrast-seed=7", "--contrast-num-phonons=1000"]
BATCHES = ["--error-batches=8"]


def command_lines():
    for p in PRODUCTS:
        yield p
        yield p + ["--job-error-batches=8"]
        yield p + BATCHES + ["--reports=ALL_ON"]
    for p, q in itertools.permutations(PRODUCTS, 2):
        yield p + q
        yield p + q + BATCHES
    for three in itertools.combinations(PRODUCTS, 3):
        yield sum(three, []) + BATCHES
    for c in COMPANIONS:
        yield [c]
        yield [c] + BATCHES + ["--slant-stack=0,0.3,8"]
        yield [c] + BATCHES + ["--lapse-windows"]


def message(args, tmp):
    """The `** Message:` line of ./main args, or None where the options were accepted (the run then fails for want of a model)."""
    r = subprocess.run([os.path.join(REPO, "main")] + args, cwd=tmp, capture_output=True, text=True, timeout=120)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("** Message:")]
    if not lines:
        return None
    assert r.returncode == 1 and len(lines) == 1, (args, r.returncode, lines)
    return lines[0]


if __name__ == "__main__":
    import tempfile
    cases = list(command_lines())
    assert len(cases) == 221 and len(COMPANIONS) == 27, (len(cases), len(COMPANIONS))
    with tempfile.TemporaryDirectory() as tmp:
        refused = [{"args": a, "message": m} for a in cases for m in [message(a, tmp)] if m is not None]
    assert len(refused) >= 200, f"only {len(refused)} of {len(cases)} command lines were refused while the options were processed"
    out = {"_provenance": "./main built from the commit before the refusals of the batched products became one loop over a "
                          "table (tests/golden/make_cli_refusals.py): argument lists and the `** Message:` line each got.",
           "cases": refused}
    with open(os.path.join(REPO, "tests", "golden", "cli_refusals.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"{len(refused)} of {len(cases)} command lines recorded")
