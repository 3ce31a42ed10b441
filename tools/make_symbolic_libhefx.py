"""Builds the fuzz of the C++ shim's recorder WITHOUT a GPU (tests/test_shim_fuzz_cpu.py):
    build/symbolic/libhefx.so   drivers/hefx_symbolic.cpp -- the symbolic stand-in for the engine -- plus one generated
                                fall-back per prototype of include/hefx.h and include/hefx_bfv.h (what seal.h names) that it does
                                not define -- the BFV entries among them, fuzz programs are CKKS: the fall-back fails by name
                                (nothing succeeds silently)
    build/symbolic/shim_fuzz    drivers/shim_fuzz.cpp linked against it
    python tools/make_symbolic_libhefx.py [--sanitize] && build/symbolic/shim_fuzz --seed 7 --dump
--sanitize builds both with -fsanitize=address,undefined into build/symbolic_san/ (a stand-alone program: nothing is
preloaded).  The library is named like the real one, so whoever builds it removes the directory afterwards."""
import os, re, subprocess, sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(root, "tools"))
from make_stub_libhefx import SHIM_HEADERS, prototypes  # noqa: E402


def main():
    sanitize = "--sanitize" in sys.argv[1:]
    out = os.path.join(root, "build", "symbolic_san" if sanitize else "symbolic")
    os.makedirs(out, exist_ok=True)
    sym = os.path.join(root, "drivers", "hefx_symbolic.cpp")
    # its definitions start a line with the return type (the file's own helpers carry no hefx_ prefix)
    defined = set(re.findall(r"^(?:int|void|const char \*|uint32_t|uint64_t) ?(hefx_[a-z0-9_]+)\(", open(sym).read(), flags=re.M))
    src = [f'#include "{name}"' for name in SHIM_HEADERS] + ["#include <cstdio>", "#include <cstdlib>", 'extern "C" {']
    missing = []
    for full, name, _ in prototypes():
        if name in defined:
            continue
        missing.append(name)
        ret = full[: full.index(name)].strip()
        loud = f'std::fprintf(stderr, "hefx-symbolic-error: symbolic: {name}: not modelled by the symbolic engine\\n");'
        if ret == "int":
            body = loud + " return HEFX_ERR_UNSUPPORTED;"
        else:  # no way to report through the return value: stop the run
            body = loud + " std::abort();"
        src.append(f"{full} {{ {body} }}")
    src.append("}")
    open(os.path.join(out, "fallbacks.cpp"), "w").write("\n".join(src) + "\n")
    inc = os.path.join(root, "include")
    san = ["-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.check_call(["g++"] + san + ["-g", "-std=c++17", "-shared", "-fPIC", "-I" + inc, sym, os.path.join(out, "fallbacks.cpp"), "-o",
                           os.path.join(out, "libhefx.so")])
    subprocess.check_call(["g++"] + san + ["-g", "-std=c++17", "-w", "-I" + inc, os.path.join(root, "drivers", "shim_fuzz.cpp"), "-o",
                           os.path.join(out, "shim_fuzz"), "-L" + out, "-lhefx", "-Wl,-rpath,$ORIGIN"])
    print(f"{out}: {len(defined)} entries modelled, {len(missing)} fail by name: {' '.join(missing)}")


if __name__ == "__main__":
    main()
