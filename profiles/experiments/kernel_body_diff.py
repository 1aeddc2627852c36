"""Compare kernel bodies of two device assembly files (hipcc --offload-arch=gfx950 -S --cuda-device-only).

usage: kernel_body_diff.py OLD.s NEW.s OLDSUB=NEWSUB [OLDSUB=NEWSUB ...]
A body is the instructions between a kernel's label and its `s_endpgm`: comments (everything behind `;`) and blank lines are dropped
and the per-function counter in local labels (.LBB3_7) is removed; the symbol's own name is not part of the body, so a changed
mangled name (an added template parameter) does not count, but any instruction, operand or register does.
Kernels are paired by substrings of their mangled names, one per file, e.g. `fast_kernelILi1ELb1EE=fast_kernelILi1ELb1ELb0EE`.
"""
import re
import sys


def bodies(path):
    out, name, cur = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):\s*(;.*)?$", line)
        if m and name is None:
            name, cur = m.group(1), []
            continue
        if name is not None:
            code = line.split(";")[0].rstrip()
            if code.strip():
                cur.append(code)
            if code.strip() == "s_endpgm":
                out[name] = cur
                name = None
    return out


def main():
    old, new = bodies(sys.argv[1]), bodies(sys.argv[2])
    bad = 0
    for key in sys.argv[3:]:
        ka, kb = key.split("=")
        a = [n for n in old if ka in n]
        b = [n for n in new if kb in n]
        if len(a) != 1 or len(b) != 1:
            print(f"{key}: ambiguous {a} {b}")
            bad += 1
            continue
        # local labels carry a per-function counter (.LBB3_7): a kernel that moved in the file renumbers them
        norm = lambda body: [re.sub(r"\.LBB\d+_", ".LBB_", l) for l in body]
        same = norm(old[a[0]]) == norm(new[b[0]])
        print(f"{key}: {len(old[a[0]])} / {len(new[b[0]])} instructions, {'identical' if same else 'DIFFERENT'}")
        bad += 0 if same else 1
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
