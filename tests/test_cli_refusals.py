"""What ./main answers when its batched products (--lapse-windows, --ttimage, --target-error, --envelope-shape, --envelope-fit,
--slant-stack, --array-contrast) are combined with each other, with --job-error-batches, with --reports or with each other's
companion options: every command line of tests/golden/cli_refusals.json (recorded by tests/golden/make_cli_refusals.py from
the ./main whose refusals were seven hand-written blocks) must still be refused with the same message -- the same rule wins
where a command line breaks several.  No command line names a model, and none needs a GPU."""
import json
import os
import subprocess

from cli_support import main_exe

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cli_refusals.json")


def test_every_recorded_command_line_is_refused_with_the_recorded_message(tmp_path):
    cases = json.load(open(GOLDEN))["cases"]
    assert len(cases) >= 200   # (the generator's own floor: the fixture cannot quietly become empty)
    wrong = []
    for case in cases:
        r = subprocess.run([main_exe()] + case["args"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("** Message:")]
        if r.returncode != 1 or got != [case["message"]]:
            wrong.append((case["args"], r.returncode, got, case["message"]))
    assert not wrong, f"{len(wrong)} of {len(cases)}; the first: {wrong[0]}"
    assert not list(tmp_path.iterdir())
