"""The host workgroup emulation of the "one workgroup per row" units: csrc/<unit>.hip compiled by the host compiler over kernels.h (this folder's stand-in
for csrc/kernels.h, which includes the shipped csrc/rowops.h) together with one of the drivers here, as a stand-alone program with its own main."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def build(tmp_dir, units, driver, headers=()):
    """Copy csrc/<unit>.hip as rgqa_amd/csrc/<unit>.cpp for every unit, the stand-in kernels.h and csrc/rowops.h beside them, `headers` (repository
    paths) to the same paths and `driver` (a file of this folder) under tmp_dir; compile the driver with the host sanitizers where the toolchain has their
    runtimes, without them where it has not.  Returns the program's path."""
    csrc = os.path.join(ROOT, "rgqa_amd", "csrc")
    dst = os.path.join(str(tmp_dir), "rgqa_amd", "csrc")
    os.makedirs(dst)
    for unit in units:
        shutil.copy(os.path.join(csrc, unit + ".hip"), os.path.join(dst, unit + ".cpp"))
    shutil.copy(os.path.join(HERE, "kernels.h"), dst)
    shutil.copy(os.path.join(csrc, "rowops.h"), dst)
    for h in headers:
        os.makedirs(os.path.join(str(tmp_dir), os.path.dirname(h)), exist_ok=True)
        shutil.copy(os.path.join(ROOT, h), os.path.join(str(tmp_dir), h))
    shutil.copy(os.path.join(HERE, driver), str(tmp_dir))
    base = ["g++", "-std=c++20", "-O1", "-pthread", "-I.", driver, "-o", "emu"]
    r = subprocess.run(base + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], cwd=str(tmp_dir), capture_output=True, text=True)
    if r.returncode != 0:          # a toolchain without the sanitizer runtimes: the same program without them
        r = subprocess.run(base, cwd=str(tmp_dir), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return os.path.join(str(tmp_dir), "emu")
