#!/usr/bin/env python3
"""Is the gfx950 device code of two builds the same, kernel by kernel?  (A host-only change reorders template instantiations: the object
files' bytes differ, the kernels must not.)

    python3 profiles/tools/compare_device_code.py OLD_BUILD_DIR NEW_BUILD_DIR [name.o ...]      (default: every *.o of OLD_BUILD_DIR)

Per object: the same symbols in the code object; every function's disassembly equal up to its last s_endpgm (comments stripped, the rest
is padding); every kernel's metadata note equal in NOTE_KEYS.  One markdown table row per object; exit status 1 on any difference."""
import os, re, subprocess, sys, tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
NOTE_KEYS = ("vgpr_count", "sgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
             "private_segment_fixed_size", "kernarg_segment_size", "max_flat_workgroup_size")

run = lambda *cmd: subprocess.run(cmd, check=True, capture_output=True, text=True).stdout      # noqa: E731

def code_object(obj, tmp):
    fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
    try:
        run(f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj, os.path.join(tmp, "copy.o"))
    except subprocess.CalledProcessError:
        return None                                          # no .hip_fatbin section: no device code in this unit
    run(f"{LLVM}/clang-offload-bundler", "--type=o", f"--targets={TARGET}", f"--input={fat}", f"--output={co}", "--unbundle")
    return co

def functions(co):
    """symbol -> instruction text up to its last s_endpgm"""
    out, name = {}, None
    for ln in run(f"{LLVM}/llvm-objdump", "-d", "--no-leading-addr", "--no-show-raw-insn", co).splitlines():
        m = re.search(r"<([^>]+)>:\s*$", ln)
        if m:
            name = m.group(1)
            out[name] = []
        elif name is not None and ln.strip():
            out[name].append(re.sub(r"\s*//.*$", "", ln).strip())
    for name, ins in out.items():
        ends = [i for i, x in enumerate(ins) if x.startswith("s_endpgm")]
        out[name] = "\n".join(ins[:ends[-1] + 1] if ends else ins)
    return out

def notes(co):
    """kernel -> the resource fields of its metadata note"""
    out, cur = {}, None
    for ln in run(f"{LLVM}/llvm-readelf", "--notes", co).splitlines():
        if re.match(r"^\s{2}- \.", ln):
            cur = {}
        m = re.match(r"^\s{2}(?:- |\s{2})\.(\w+):\s+(.*)$", ln)
        if m and cur is not None:
            if m.group(1) == "name":
                out[m.group(2).strip("'\"")] = cur
            elif m.group(1) in NOTE_KEYS:
                cur[m.group(1)] = m.group(2)
    for k, v in out.items():      # (a changed layout of the notes' text must not read as "nothing to compare")
        assert set(v) == set(NOTE_KEYS), f"{co}: note of {k} lacks {sorted(set(NOTE_KEYS) - set(v))}"
    return out

def compare(old, new):
    with tempfile.TemporaryDirectory() as t0, tempfile.TemporaryDirectory() as t1:
        a, b = code_object(old, t0), code_object(new, t1)
        if a is None or b is None:
            return (a is None) == (b is None), 0, "no device code"
        fa, fb, na, nb = functions(a), functions(b), notes(a), notes(b)
    bad = []
    if set(fa) != set(fb) or set(na) != set(nb):
        bad.append("symbols differ: " + ", ".join(sorted((set(fa) ^ set(fb)) | (set(na) ^ set(nb))))[:300])
    bad += [f"code differs: {k}" for k in sorted(set(fa) & set(fb)) if fa[k] != fb[k]]
    bad += [f"note differs: {k} {na[k]} -> {nb[k]}" for k in sorted(set(na) & set(nb)) if na[k] != nb[k]]
    assert na and set(na) <= set(fa), f"{new}: kernels without code"
    return not bad, len(na), "; ".join(bad) if bad else f"{len(fa)} functions, {sum(x.count(chr(10)) + 1 for x in fa.values())} instructions equal"

if __name__ == "__main__":
    old_dir, new_dir = sys.argv[1], sys.argv[2]
    ok_all = True
    print("| object | kernels | symbols, code, notes |\n|---|---|---|")
    for n in sys.argv[3:] or sorted(f for f in os.listdir(old_dir) if f.endswith(".o")):
        ok, kernels, text = compare(os.path.join(old_dir, n), os.path.join(new_dir, n))
        ok_all &= ok
        print(f"| {n} | {kernels} | {'same' if ok else 'DIFFERENT'}: {text} |")
    sys.exit(0 if ok_all else 1)
