"""Kernel-by-kernel comparison of the GEMM units' gfx950 code between two builds (no GPU needed):

    python tools/gemm_isa_diff.py <dir with the other build's objects> [<dir with this build's objects>] [--md] [--units=a,b] [--alias=OLD=NEW ...]

Each directory holds <unit>.o as rgqa_amd/build.py (rgqa_amd/csrc/build, the default for the second) or tools/build_variant.sh (its object
directory) leaves them.  Per unit the gfx950 code object is unbundled (as tools/kernel_regs.sh does) and disassembled; a kernel's stream is
its instructions' text with addresses and encodings dropped.  Printed per kernel: instruction count, VALU (v_* other than MFMA), MFMA, VGPR,
AGPR, SGPR, LDS bytes, scratch bytes of either build and whether the two streams are equal instruction for instruction; then the kernels that
exist in one build only.  --alias=OLD=NEW compares the other build's kernel OLD with this build's NEW (a renamed kernel); names as printed."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/lib/llvm/bin")
UNITS = ("gemm_mfma", "gemm_mfma256", "gemm_x3", "gemm_f32")


def kernels(obj):
    """{demangled kernel name: (instruction texts, metadata dict)} of one object"""
    with tempfile.TemporaryDirectory() as t:
        fat, co = os.path.join(t, "fat.bin"), os.path.join(t, "k.co")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj], check=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
        dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], check=True, capture_output=True, text=True).stdout
    meta = {}
    for k in re.split(r"\n\s+- \.agpr_count", "\n" + notes)[1:]:
        k = ".agpr_count" + k
        g = lambda f: int(re.search(r"\." + f + r":\s+(\d+)", k).group(1))
        meta[re.search(r"\.name:\s+(\S+)", k).group(1)] = dict(vgpr=g("vgpr_count"), agpr=g("agpr_count"), sgpr=g("sgpr_count"),
                                                               lds=g("group_segment_fixed_size"), scratch=g("private_segment_fixed_size"))
    streams, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = m.group(1) if m.group(1) in meta else None
            if cur:
                streams[cur] = []
            continue
        if cur and line.startswith("\t"):
            streams[cur].append(re.sub(r"\s*//.*$", "", line).strip())
    names = sorted(streams)
    filt = shutil.which("llvm-cxxfilt", path=LLVM) or shutil.which("c++filt")       # without either the names stay mangled
    # DF16b (__bf16) is newer than some demanglers: hand it over as a vendor type named bf16
    dem = subprocess.run([filt] + [n.replace("DF16b", "u4bf16") for n in names], check=True, capture_output=True, text=True).stdout.splitlines() if filt and names else names
    out = {}
    for n, d in zip(names, dem):
        ins = streams[n]
        while ins and ins[-1].startswith("s_nop") or ins and ins[-1].startswith("s_code_end"):     # padding behind s_endpgm
            ins.pop()
        out[re.sub(r"^void ", "", re.sub(r"\(.*$", "", d))] = (ins, meta[n])
    return out


def counts(ins):
    mfma = sum(1 for i in ins if i.startswith("v_mfma"))
    return len(ins), sum(1 for i in ins if i.startswith("v_")) - mfma, mfma


def main():
    dirs = [a for a in sys.argv[1:] if not a.startswith("--")]
    units = UNITS
    for a in sys.argv[1:]:
        if a.startswith("--units="):
            units = a[len("--units="):].split(",")
    alias = dict(a[len("--alias="):].split("=", 1) for a in sys.argv[1:] if a.startswith("--alias="))
    old_dir, new_dir = dirs[0], (dirs[1] if len(dirs) > 1 else os.path.join(ROOT, "rgqa_amd", "csrc", "build"))
    md = "--md" in sys.argv
    hdr = ("unit", "kernel", "instr", "VALU", "MFMA", "VGPR", "AGPR", "SGPR", "LDS", "scratch", "stream")
    if md:
        print("| " + " | ".join(hdr) + " |")
        print("|" + "---|" * len(hdr))
    same = differ = 0
    only = []
    for u in units:
        old, new = kernels(os.path.join(old_dir, u + ".o")), kernels(os.path.join(new_dir, u + ".o"))
        old = {alias.get(k, k): v for k, v in old.items()}
        for name in sorted(set(old) | set(new)):
            if name not in old or name not in new:
                only.append((u, name, "other build only" if name in old else "this build only"))
                continue
            (io, mo), (im, mn) = old[name], new[name]
            eq = io == im
            same, differ = same + eq, differ + (not eq)
            co, cn = counts(io), counts(im)
            pair = lambda a, b: str(a) if a == b else "%s -> %s" % (a, b)
            vals = [u, name] + [pair(a, b) for a, b in zip(co, cn)] + [pair(mo[k], mn[k]) for k in ("vgpr", "agpr", "sgpr", "lds", "scratch")] + ["equal" if eq else "DIFFERS"]
            print(("| %s | `%s` | " % (vals[0], vals[1]) + " | ".join(vals[2:]) + " |") if md else "  ".join(vals))
    print()
    print("%d kernels in both builds: %d instruction-for-instruction equal, %d differ" % (same + differ, same, differ))
    for u, name, where in only:
        print("%s: %s: `%s`" % (where, u, name))


if __name__ == "__main__":
    main()
