"""Kernel-by-kernel comparison of two device assembly files of one source, to show that a refactor
left the device code alone.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S FILE.hip -o FILE.s    (both trees)
    python tools/asm_kernel_diff.py OLD.s NEW.s [--rename REGEX=TEXT]

A function is everything from its ``.type NAME,@function`` line to its ``.size NAME`` line: labels,
instructions and, for a kernel, its descriptor (register counts, LDS and scratch sizes).  Comments are
dropped, as are section and linkage directives, and the function's number in local labels is masked;
the rest is compared as text.  ``--rename`` rewrites names of OLD first (a kernel that lost a template
parameter).  Prints one line per function that differs or exists on one side only -- with the
opcodes that were inserted or deleted, registers and operands aside -- then the counts; exit status 1
if any differ.
"""
import difflib
import re
import sys


def functions(path, rename=None):
    out, name, body = {}, None, []
    for line in open(path, errors="replace"):
        if rename:
            line = rename[0].sub(rename[1], line)
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            name, body = m.group(1), []
        if name is None:
            continue
        code = re.sub(r"\.L(BB|func_end|func_begin|tmp)\d+", r".L\1", line.split(";", 1)[0]).rstrip()
        if code.strip() and not re.match(r"\s*\.(section|text|globl|weak|protected|hidden)\b", code):
            body.append(code)
        if re.match(r"\s*\.size\s+%s," % re.escape(name), line):
            out[name], name = body, None
    return out


def main():
    argv = sys.argv[1:]
    rename = None
    if "--rename" in argv:
        i = argv.index("--rename")
        rx, to = argv[i + 1].split("=", 1)
        rename = (re.compile(rx), to)
        del argv[i:i + 2]
    old, new = functions(argv[0], rename), functions(argv[1])
    same = diff = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print("%s: only in %s" % (name, "OLD" if name in old else "NEW"))
            diff += 1
        elif old[name] != new[name]:
            a, b = old[name], new[name]
            nd = sum(1 for x, y in zip(a, b) if x != y) + abs(len(a) - len(b))
            first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            print("%s: %d of %d / %d lines differ, first: %r | %r" % (
                name, nd, len(a), len(b), a[first].strip() if first < len(a) else None,
                b[first].strip() if first < len(b) else None))
            ops = [[ln.split()[0] for ln in x if not re.match(r"\s*(\.|\S+:$)", ln)] for x in (a, b)]
            edits = [o for o in difflib.SequenceMatcher(None, ops[0], ops[1], autojunk=False).get_opcodes()
                     if o[0] != "equal"]
            gone = sorted(set(m for o in edits for m in ops[0][o[1]:o[2]]))
            came = sorted(set(m for o in edits for m in ops[1][o[3]:o[4]]))
            print("    opcodes: %d / %d, %d edits between instructions %d and %d; deleted %s, inserted %s" % (
                len(ops[0]), len(ops[1]), len(edits), edits[0][1] if edits else -1, edits[-1][2] if edits else -1,
                gone, came))
            diff += 1
        else:
            same += 1
    print("identical: %d  different: %d" % (same, diff))
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
