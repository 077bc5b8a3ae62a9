#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds, per kernel, on the CPU.

    for f in csrc/*.hip; do hipcc --offload-arch=gfx950 --cuda-device-only -S $CXXFLAGS $f -o DIR/$(basename $f .hip).s; done
    tools/kernel_diff.py OLD_DIR NEW_DIR [--only REGEX] [--map old_symbol=new_symbol ...] [--json OUT]

Prints, for every kernel of OLD_DIR (paired by symbol, or through --map where it was renamed or moved to another file):
VGPRs, SGPRs, static LDS, scratch and spills from the code object metadata, the instruction count, and whether the
instruction streams are identical once comments and directives are gone, local labels are renumbered in order of
appearance and the kernel's own symbol is masked.  Exit status 1 where a pair differs in body or metadata."""
import argparse, difflib, glob, json, os, re, sys

META = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count",
        "sgpr_spill_count")


def kernels(directory):
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        text = open(path).read()
        metas, cur = {}, None
        for line in text.split("amdhsa.kernels:", 1)[-1].splitlines():
            m = re.match(r"^  (- | {2})\.(\w+):\s*(\S*)$", line)
            if m and m.group(1) == "- ":
                cur = {}
            if m and cur is not None:
                cur[m.group(2)] = m.group(3).strip("'\"")
                if m.group(2) == "name":
                    metas[cur["name"]] = cur
        lines = text.splitlines()
        for sym, meta in metas.items():
            body, labels = [], {}
            start = next(i for i, l in enumerate(lines) if l.startswith(sym + ":"))
            for line in lines[start + 1:]:
                if line.startswith(".Lfunc_end"):
                    break
                line = line.split(";", 1)[0].strip()
                if not line or (line.startswith(".") and not line.endswith(":")):
                    continue
                line = re.sub(r"\.L\w+", lambda m: labels.setdefault(m.group(0), "L%d" % len(labels)), line)
                body.append(line.replace(sym, "KERNEL"))
            out[sym] = {"file": os.path.basename(path), "meta": {k: int(meta.get(k, 0)) for k in META},
                        "instructions": sum(not l.endswith(":") for l in body), "body": body}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old"), ap.add_argument("new")
    ap.add_argument("--only", default="", help="regex on the old symbol")
    ap.add_argument("--map", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("--json", help="write the table here")
    ap.add_argument("--diff", action="store_true", help="print the differing lines of a pair")
    args = ap.parse_args()
    old, new, ren = kernels(args.old), kernels(args.new), dict(m.split("=", 1) for m in args.map)
    rows, bad = [], 0
    for sym in sorted(s for s in old if re.search(args.only, s)):
        o, n = old[sym], new.get(ren.get(sym, sym))
        if n is None:
            print("%-70s only in %s" % (sym, args.old))
            bad += 1
            continue
        differing = sum(a != b for a, b in zip(o["body"], n["body"])) + abs(len(o["body"]) - len(n["body"]))
        same_meta = o["meta"] == n["meta"]
        bad += bool(differing) or not same_meta
        rows.append({"old": sym, "new": ren.get(sym, sym), "old_meta": o["meta"], "new_meta": n["meta"],
                     "old_instructions": o["instructions"], "new_instructions": n["instructions"],
                     "identical_body": not differing, "differing_lines": differing})
        print("%s\n    %s | instructions %d -> %d | %s%s" % (
            sym, " ".join("%s %d->%d" % (k.replace("_count", "").replace("_fixed_size", ""), o["meta"][k], n["meta"][k]) for k in META),
            o["instructions"], n["instructions"], "IDENTICAL" if not differing else "%d lines differ" % differing,
            "" if same_meta else " | METADATA DIFFERS"))
        if args.diff and differing:
            print("\n".join(difflib.unified_diff(o["body"], n["body"], "old", "new", n=2, lineterm="")))
    if args.json:
        json.dump(rows, open(args.json, "w"), indent=1)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
