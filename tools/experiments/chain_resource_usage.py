#!/usr/bin/env python
"""Resource figures and instruction-stream fingerprints of the denoiser kernels from hipcc's -S output, in the columns of
profiles/chain_kernels_resource_usage.txt: VGPR, AGPR, SGPR, spilled scalars, spilled vector registers, scratch bytes per lane, occupancy,
instruction lines of the body, SHA-1 of the body with basic-block labels normalised (equal sha = equal instruction stream), packed-fp32 count.

    python tools/experiments/chain_resource_usage.py [--asm new.s] [--against old.s] [--src difffacto_amd/csrc/denoiser_kernel.hip]

With --against, every kernel of the first listing is compared with the kernel of the same name in the second one.  A template argument that
changed its type but not its value (`Lb0` <-> `Li0`) names the same kernel: the chain kernels' FROM flag became the ChainKind 0 / 1 / 2."""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

KINDS = {"0": "", "1": ", FROM", "2": ", PLAIN"}


def pretty(sym):
    """_ZN12_GLOBAL__N_114k_denoise_pipeILi8ELi2EEEvNS_7KParamsE -> k_denoise_pipe<8, PLAIN>"""
    m = re.search(r"\d+(k_[a-z0-9_]+?)I((?:L[ib]\d+E)+)E", sym)
    if not m:
        return sym
    name, args = m.group(1), re.findall(r"L[ib](\d+)E", m.group(2))
    if name == "k_denoise":   # <PREC, NW, FROM>
        return "k_denoise<%s%s>" % ("f32" if args[0] == "0" else "bf16", KINDS[args[2]])
    if name in ("k_denoise_coop", "k_denoise_coop2"):
        return name + ("<%s>" % KINDS[args[0]][2:] if KINDS[args[0]] else "")
    return "%s<%s%s>" % (name, args[0], KINDS[args[1]])


def compile_asm(src, flags):
    from difffacto_amd import build as b
    asm = os.path.join(tempfile.gettempdir(), "chain_resource_usage.s")
    cmd = [b._hipcc(), *b.FLAGS, *flags, "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "difffacto_amd", "csrc"), "-S", "--cuda-device-only",
           "-o", asm, src]
    subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
    return asm


def kernels(asm):
    """{pretty name: dict of figures} for every k_denoise* kernel of the listing."""
    text = open(asm).read()
    lines = text.split("\n")
    out = {}
    spills = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", text):
        spills[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    i = 0
    while i < len(lines):
        m = re.match(r"^(_Z\w*k_denoise\w*):", lines[i])
        if not m:
            i += 1
            continue
        sym = m.group(1)
        body, labels = [], {}
        j = i + 1
        while not lines[j].startswith("\t.section") and ".Lfunc_end" not in lines[j]:
            l = lines[j].split(";")[0].rstrip() if not lines[j].lstrip().startswith(";;#") else lines[j].rstrip()
            j += 1
            s = l.strip()
            if not s or s.startswith("."):
                lab = re.match(r"^(\.LBB\d+_\d+):", s)
                if not lab:
                    continue
                labels.setdefault(lab.group(1), "L%d" % len(labels))
            body.append(s)
        norm = []
        for s in body:
            for lab in re.findall(r"\.LBB\d+_\d+", s):
                labels.setdefault(lab, "L%d" % len(labels))
            norm.append(re.sub(r"\.LBB\d+_\d+", lambda q: labels[q.group(0)], s))
        insts = [s for s in norm if not re.match(r"^L\d+:$", s) and not s.startswith(";;#")]
        info = {}
        while j < len(lines) and not lines[j].startswith("; Occupancy"):
            q = re.match(r"^; (TotalNumSgprs|NumVgprs|NumAgprs|ScratchSize): (\d+)", lines[j])
            if q:
                info[q.group(1)] = int(q.group(2))
            j += 1
        info["Occupancy"] = int(lines[j].split(":")[1])
        sg, vg = spills.get(sym, (-1, -1))
        out[pretty(sym)] = dict(vgpr=info["NumVgprs"], agpr=info["NumAgprs"], sgpr=info["TotalNumSgprs"], sspill=sg, vspill=vg, scratch=info["ScratchSize"],
                                occ=info["Occupancy"], insts=len(insts), sha=hashlib.sha1("\n".join(norm).encode()).hexdigest()[:10],
                                pk=sum(1 for s in insts if re.match(r"v_pk_(fma|add|mul)_f32", s)))
        i = j
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm", default=None, help="existing -S listing (default: compile --src)")
    ap.add_argument("--against", default=None, help="a second listing to compare with, kernel by kernel")
    ap.add_argument("--src", default=os.path.join(ROOT, "difffacto_amd/csrc/denoiser_kernel.hip"))
    ap.add_argument("--flags", default="")
    ap.add_argument("--state", default="", help="text of the `state` column")
    args = ap.parse_args()
    new = kernels(args.asm or compile_asm(args.src, args.flags.split()))
    old = kernels(args.against) if args.against else {}
    print("kernel".ljust(29) + "state".ljust(36) + "VGPR  AGPR  SGPR SGPR spill VGPR spill scratch B/lane occupancy  insts  sha")
    for name, k in new.items():
        row = (name.ljust(29) + args.state.ljust(34) + "%6d%6d%6d%11d%11d%15d%10d%7d  %s  v_pk_*_f32 %d" %
               (k["vgpr"], k["agpr"], k["sgpr"], k["sspill"], k["vspill"], k["scratch"], k["occ"], k["insts"], k["sha"], k["pk"]))
        if name in old:
            row += "  = the other listing's" if old[name]["sha"] == k["sha"] else "  differs (%d insts there, sha %s)" % (old[name]["insts"], old[name]["sha"])
        elif old:
            row += "  (not in the other listing)"
        print(row)


if __name__ == "__main__":
    main()
