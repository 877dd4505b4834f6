"""Compare the gfx950 kernels of two builds of the library instruction by instruction.

    python tools/rigid_disasm_diff.py OLD.so NEW.so [--show N]

Every kernel symbol of OLD is disassembled in both libraries (llvm-objdump, no addresses, no encodings; branch targets and
PC-relative constants reduced to placeholders; the alignment fill behind a function's last instruction dropped: a template
kernel sits in a section of its own, a plain one is padded up to its neighbour) and the instruction lists are compared.  Prints how many are identical,
which differ (by family), which are missing from NEW and which are new in NEW.  Used to show that adding the scaled kernels
left every rigid kernel as it was (CHANGELOG.md).

k_solve, k_classify, k_reduce and k_debug_sdf_at are paired across the fold of each rigid / scaled kernel pair into one
template: k_X<...> of a build with twins is k_X<...> with an empty scale pack, its k_X_sc<...> is k_X<..., ScaleDev>.
"""
import collections
import difflib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tests", "test_kernel_resources.py"))
kr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kr)


PAIRED = ("k_solve", "k_classify", "k_reduce", "k_debug_sdf_at")


def canon(sym):
    """'k_solve<6, 2, 1>' / 'k_solve<6, 2, 1, ScaleDev>' for a kernel of the four paired stages under either naming (the
    mangled argument list differs between the two, the template arguments do not); every other symbol as it is."""
    m = re.match(r"_ZN5svsdf(\d+)", sym)
    if not m:
        return sym
    end = m.end() + int(m.group(1))
    name, rest = sym[m.end():end], sym[end:]
    base = name[:-3] if name.endswith("_sc") else name
    if base not in PAIRED:
        return sym
    t = re.match(r"I((?:Li\d+E)*)(JE|JNS_8ScaleDevEE)?E", rest)
    args = re.findall(r"Li(\d+)E", t.group(1)) if t else []
    if name.endswith("_sc") or (t and t.group(2) == "JNS_8ScaleDevEE"):
        args.append("ScaleDev")
    return f"{base}<{', '.join(args)}>"


def functions(lib):
    out = {}
    for co in kr.code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            txt = subprocess.run([kr._tool("llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", f.name],
                                 check=True, stdout=subprocess.PIPE).stdout.decode()
        cur = None
        for line in txt.splitlines():
            m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", line)
            if m:
                cur = canon(m.group(1))
                out.setdefault(cur, [])
                continue
            if cur is None or not line.strip():
                continue
            line = re.sub(r"//.*$", "", line).rstrip()
            if "s_getpc" in line or "branch" in line:
                line = re.sub(r"0x[0-9a-f]+", "ADDR", line)
            out[cur].append(re.sub(r"<[^>]*>", "<L>", line).strip())
    for body in out.values():   # fill between functions (objdump lists it under the symbol before it): not the kernel's
        while body and body[-1] in ("s_nop 0", "..."):
            body.pop()
    return out


def family(sym):
    if sym.split("<")[0] in PAIRED:
        return sym.split("<")[0] + (" (scaled)" if "ScaleDev" in sym else "")
    m = re.search(r"(k_\w+?)(?:I|E)", sym)
    return m.group(1) if m else sym[:40]


def main():
    old, new = functions(sys.argv[1]), functions(sys.argv[2])
    show = int(sys.argv[sys.argv.index("--show") + 1]) if "--show" in sys.argv else 0
    diff = [k for k in old if k in new and old[k] != new[k]]
    missing = [k for k in old if k not in new]
    added = [k for k in new if k not in old]
    print(f"kernels in {os.path.basename(sys.argv[1])}: {len(old)}; identical: {len(old) - len(diff) - len(missing)}; "
          f"differing: {len(diff)}; missing: {len(missing)}; new: {len(added)}")
    print("differing by family:", dict(collections.Counter(family(k) for k in diff)))
    print("new by family:", dict(collections.Counter(family(k) for k in added)))
    for k in diff[:show]:
        d = [l for l in difflib.unified_diff(old[k], new[k], lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---")]
        print(f"{k}: {len(d)} lines differ")
        print("\n".join(d[:12]))


if __name__ == "__main__":
    main()
