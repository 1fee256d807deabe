"""Are the kernels of two device-assembly files the same machine code?
  python scripts/kernel_asm_diff.py old.s new.s [--gone REGEX]
The .s files come from the Makefile's flags with -S --cuda-device-only (tests/test_host_cpu.py builds them the same way).
Per kernel symbol (and per device function left out of line), the text from its label to the end of its .amdhsa_kernel block (instructions, registers, LDS, scratch,
occupancy fields) is compared after dropping line-marker directives and renumbering the compiler's local labels
(.LBB<fn>_<blk>, .Lfunc_end<fn>, .Lpost_getpc<n>), whose numbers shift when a function before them leaves the file.
Exit status 0: every kernel of new.s is in old.s and identical, and the kernels only in old.s all match --gone."""
import re
import sys


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n.*?^\t\.end_amdhsa_kernel\n", text, re.M | re.S):
        name = m.group(1)
        start = text.index(f"\n{name}:") + 1
        out[name] = normalise(text[start:m.end()])
    # device functions the kernels call without inlining them: label to .Lfunc_end
    for m in re.finditer(r"^\t\.type\t(\S+),@function\n", text, re.M):
        if m.group(1) not in out:
            start = text.index(f"\n{m.group(1)}:") + 1
            out[m.group(1)] = normalise(text[start:text.index("\n.Lfunc_end", start)])
    return out


def normalise(body):
    lines = [l for l in body.split("\n") if not re.match(r"\s*\.(loc|file|cfi_\w+)\b", l)]
    body = re.sub(r"\bL?BB\d+_", "BB_", "\n".join(lines))       # labels, and the loop comments that name them
    body = re.sub(r"[ \t]+;", " ;", body)                                  # comment columns move with a label's width
    body = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", body)
    seen = {}
    return re.sub(r"\.Lpost_getpc\d+", lambda m: f".Lpost_getpc#{seen.setdefault(m.group(0), len(seen))}", body)


if __name__ == "__main__":
    args = sys.argv[1:]
    gone_re = args[args.index("--gone") + 1] if "--gone" in args else None
    old, new = kernels(args[0]), kernels(args[1])
    added = sorted(set(new) - set(old))
    gone = sorted(set(old) - set(new))
    differ = sorted(k for k in new if k in old and new[k] != old[k])
    unexpected = [k for k in gone if not (gone_re and re.search(gone_re, k))]
    for title, names in (("only in new", added), ("only in old", gone), ("DIFFERENT", differ)):
        for k in names:
            print(f"{title}: {k}")
    print(f"{args[1]}: {len(new)} kernels and device functions, {len(new) - len(differ) - len(added)} identical to {args[0]} ({len(old)}), "
          f"{len(differ)} different, {len(added)} added, {len(gone)} gone ({len(unexpected)} of them unexpected)")
    sys.exit(1 if differ or added or unexpected else 0)
