"""The two ways a test gets native code built: a target of the repository's Makefile, and a few lines of C++ over one of
the project's headers compiled by the host compiler.  Either shows the tool's own output when it fails."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(cmd):
    done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    if done.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)}: exit status {done.returncode}\n" + "\n".join(done.stdout.splitlines()[-40:]))


def make(*goal, missing=None):
    """`make <goal>` at the repository's root (make decides what is stale); with `missing`, only when that file is not
    there -- what __graft_entry__.build() makes through `make all`, in a tree that was built otherwise."""
    if missing is None or not os.path.exists(missing):
        _run(["make", "-C", REPO, "-j8", *goal])
    assert missing is None or os.path.exists(missing), f"make {' '.join(goal)} did not produce {missing}"
    return missing


def host_build(directory, name, source, include, flags=("-O2", "-fPIC", "-shared"), link=()):
    """`source` (C++ text) written into `directory` and compiled to directory/name with -Wall -Werror: `include` the
    directories it finds the project's headers in, `flags` what makes it the library or program the test wants, `link`
    what follows the source on the command line.  The path of what was built."""
    src, out = os.path.join(str(directory), "wrap.cpp"), os.path.join(str(directory), name)
    with open(src, "w") as f:
        f.write(source)
    _run(["g++", "-std=c++17", *flags, "-Wall", "-Werror", *[x for d in include for x in ("-I", d)], "-o", out, src, *link])
    return out
