"""Static instruction counts of the attention kernels: compiles attn_x3.hip and attn_mfma.hip (the split-f32 and the bf16 instantiation of
csrc/attn_core.h, where the kernels' code lives; before that header each unit held its own copy) to gfx950 assembly with the flags of
rgqa_amd/build.py and prints, per kernel, what the instruction-issue cost is made of (no GPU needed):

    python tools/attn_isa_counts.py [name-filter] [--md] [--notrim] [--csrc=DIR]

--csrc=DIR reads the two units (and their headers) from DIR instead of rgqa_amd/csrc: another commit's sources beside this tree's, with or
without attn_core.h - the kernels keep their names, which is all short() relies on.

columns: instructions (everything between the kernel's label and its last s_endpgm), VALU (v_* other than MFMA), v_mul_lo_u32 (+ v_mad_u64_u32:
the quarter-rate integer multiplies), MFMA, s_nop, VGPR + AGPR, LDS bytes, scratch bytes, waves per SIMD (the compiler's occupancy figure).
A kernel with per-sample tile counts (rgqa_debug_set key 23) holds several bodies of which a wave runs ONE: its row is the sum of them.
With --notrim the units are compiled with -DATTN_NO_TRIM, every kernel then holds exactly the body of its own tile counts: the length of the
stream a wave of that shape issues."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgqa_amd import build as B  # noqa: E402

UNITS = ("attn_x3.hip", "attn_mfma.hip")


def csrc():
    for a in sys.argv[1:]:
        if a.startswith("--csrc="):
            return a[len("--csrc="):]
    return B.CSRC


def assemble(unit, out):
    flags = [f for f in B.FLAGS if f != "-fPIC"] + B.PER_FILE_FLAGS.get(unit, []) + (["-DATTN_NO_TRIM"] if "--notrim" in sys.argv else [])
    cmd = [B.HIPCC] + flags + ["-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-S", os.path.join(csrc(), unit), "-o", out]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)


def short(name):
    """_Z18attn_fwd_x3_kernelILi3ELi3EEv8AttnArgs -> attn_fwd_x3_kernel<3,3> (the only mangling these two units produce)"""
    m = re.match(r"_Z\d+([A-Za-z_]\w*?)I((?:Li\d+E)+)E", name)
    return "%s<%s>" % (m.group(1), ",".join(re.findall(r"Li(\d+)E", m.group(2)))) if m else name


def parse(path):
    rows, cur, ins = [], None, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur, ins = m.group(1), dict(n=0, valu=0, mul=0, mfma=0, nop=0)
            continue
        if cur is None:
            continue
        s = line.strip()
        if line.startswith("\t") and s and s[0].isalpha() and not s.startswith(".") and ins.get("open", True):
            op = s.split()[0]
            ins["n"] += 1
            if op.startswith("v_mfma"):
                ins["mfma"] += 1
            elif op.startswith("v_"):
                ins["valu"] += 1
            if op in ("v_mul_lo_u32", "v_mul_hi_u32", "v_mad_u64_u32", "v_mad_i64_i32", "v_mul_lo_i32"):
                ins["mul"] += 1
            if op == "s_nop":
                ins["nop"] += 1
        if s.startswith(".amdhsa_kernel"):
            ins["open"] = False
        for key, pat in (("vgpr", r"; NumVgprs: (\d+)"), ("agpr", r"; NumAgprs: (\d+)"), ("scratch", r"; ScratchSize: (\d+)"),
                         ("occ", r"; Occupancy: (\d+)"), ("lds", r"; LDSByteSize: (\d+)")):
            mm = re.match(pat, s)
            if mm:
                ins[key] = int(mm.group(1))
        if s.startswith("; Occupancy"):
            rows.append((cur, ins))
            cur = None
    return rows


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    flt = args[0] if args else ""
    md = "--md" in sys.argv
    out = []
    with tempfile.TemporaryDirectory() as t:
        for u in UNITS:
            s = os.path.join(t, u[:-4] + ".s")
            assemble(u, s)
            out += parse(s)
    names = [short(r[0]) for r in out]
    hdr = ("kernel", "instr", "VALU", "mul32", "MFMA", "s_nop", "VGPR+AGPR", "LDS", "scratch", "waves/SIMD")
    if md:
        print("| " + " | ".join(hdr) + " |")
        print("|" + "---|" * len(hdr))
    else:
        print("%-44s %6s %6s %6s %5s %6s %10s %6s %7s %10s" % hdr)
    for name, (_, i) in sorted(zip(names, out)):
        if flt and flt not in name:
            continue
        regs = "%d+%d" % (i.get("vgpr", 0), i.get("agpr", 0))
        vals = (name, i["n"], i["valu"], i["mul"], i["mfma"], i["nop"], regs, i.get("lds", 0), i.get("scratch", 0), i.get("occ", 0))
        if md:
            print("| `%s` | " % vals[0] + " | ".join(str(v) for v in vals[1:]) + " |")
        else:
            print("%-44s %6d %6d %6d %5d %6d %10s %6d %7d %10d" % vals)


if __name__ == "__main__":
    main()
