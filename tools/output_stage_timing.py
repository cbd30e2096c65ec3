"""The output stage of ./main for BASELINE config 5, three ways: the raw grid file only, with --scatter-views added, and
with --scatter-views --no-scatter-grid-file.
    python tools/output_stage_timing.py [histories=12500000] [toa_degree=9]
Prints, per form, the wall time of the whole program and of its output stage -- from the "Shards:" line, which ./main
prints when the run and the reduction of the bins are over, to the program's end (stdout line-buffered) -- and the
files left.  Files go to a temporary directory that is removed."""
import os, shutil, subprocess, sys, tempfile, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from radiative3d_amd.configs import crustpinch_vids

n = int(sys.argv[1]) if len(sys.argv) > 1 else 12_500_000
deg = int(sys.argv[2]) if len(sys.argv) > 2 else 9
base = crustpinch_vids(deg) + [f"--num-phonons={n}", "--scatter-grid=256,256,64,300,-1000,-1000,-250,1000,1000,0"]
for name, extra in (("raw file only", []), ("+ --scatter-views", ["--scatter-views"]),
                    ("--scatter-views --no-scatter-grid-file", ["--scatter-views", "--no-scatter-grid-file"])):
    out = tempfile.mkdtemp(prefix="r3d_stage_")
    t0 = time.perf_counter(); mark = None
    p = subprocess.Popen(["stdbuf", "-oL", os.path.join(REPO, "main")] + base + extra + ["--output-dir=" + out],
                         stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, cwd=out)
    for line in p.stdout:
        if "Shards:" in line: mark = time.perf_counter()
    rc = p.wait(); t1 = time.perf_counter()
    sizes = {f: os.path.getsize(os.path.join(out, f)) for f in sorted(os.listdir(out)) if "scatter" in f}
    print(f"{name}: rc {rc}, whole program {t1 - t0:.2f} s, output stage {t1 - (mark or t0):.2f} s, files {sizes}", flush=True)
    shutil.rmtree(out, ignore_errors=True)
