"""The device-free host logic (csrc/eqds_host.hpp: the bookkeeping and checks of the ProjEquiRect data set; csrc/cg_host.hpp: the end of a CG solve
for both flag layouts) through its stand-alone programme tests/c_abi/eqds_host.cpp, built with the plain host compiler.  No sanitizer flags here: the
suite also runs where a library is preloaded into every process, and a sanitizer-linked executable aborts on link order there; the sanitizer build
is the command in the programme's header, run by hand."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_programme_builds_and_passes(tmp_path):
    exe = str(tmp_path / "eqds_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "c_abi", "eqds_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "eqds_host: ok", r.stdout + r.stderr
