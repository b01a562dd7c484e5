"""Build libcfen_hip.so for gfx950 with hipcc (in-tree, so the .so travels to the GPU box)."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libcfen_hip.so")
SOURCES = ["k_gemm.hip", "k_attention.hip", "k_padnorm.hip","k_tokens.hip", "k_conv.hip", "k_conv_tile.hip", "k_mlp.hip", "k_embed.hip", "k_lvit.hip", "k_stream.hip", "k_gvit.hip", "k_head5.hip", "k_fuse.hip", "k_tail.hip", "k_tile.hip", "k_ensemble.hip", "k_resample.hip", "k_guided.hip", "k_temporal.hip", "k_motion.hip", "k_subpel.hip", "k_flicker.hip", "k_metrics.hip", "k_planes.hip", "k_colordiff.hip", "k_noref.hip", "k_yuv.hip", "k_yuv16.hip", "k_png.hip", "k_dcn.hip", "k_dcn_bwd.hip", "cfen_api.cpp", "cfen_net.cpp", "cfen_tune.cpp"]
# per-file codegen flags.  k_attention: the softmax is VALU bound -- drop fmaxf's NaN canonicalisation (no NaNs can
# occur: masked scores are -1e30, not -inf) and let MFMA results land in VGPRs instead of AGPR + v_accvgpr_read.
EXTRA_FLAGS = {"k_attention.hip": ["-fno-honor-nans", "-mllvm", "-amdgpu-mfma-vgpr-form=1"],
               # round 3: the same canonicalisation (a v_max_f32 x, x, x in front of every fmaxf operand that comes out of an MFMA) was
               # 136 of the 812 vector instructions per head and wave of k_lvit_window's attention loop, and sits in front of every ReLU
               # of the conv / GEMM epilogues
               "k_lvit.hip": ["-fno-honor-nans"], "k_mlp.hip": ["-fno-honor-nans"], "k_conv_tile.hip": ["-fno-honor-nans"],
               "k_conv.hip": ["-fno-honor-nans"], "k_gemm.hip": ["-fno-honor-nans"], "k_gvit.hip": ["-fno-honor-nans"], "k_head5.hip": ["-fno-honor-nans"], "k_fuse.hip": ["-fno-honor-nans"], "k_tail.hip": ["-fno-honor-nans"]}
# every file: no packed-fp32 VALU code (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32).  WHY, honestly: round 1 attributed a run-to-run
# nondeterminism of the two-lane plan to these instructions ("wrong high lane beside another kernel's MFMA waves").  Round 2 tested that
# claim (tools/repro_pk_fma.py, profiles/r02_pk_fma_repro.json): a stand-alone v_pk_fma_f32 / v_pk_mul_f32 kernel beside an MFMA kernel
# shows 0 mismatches in 180 launches, and this library built WITH packed-fp32 code generation (6713 such instructions) is bit-reproducible
# over 60 eager + graph forwards under GEMM noise, exactly like the shipped build.  The claim is RETRACTED: what fixed the nondeterminism
# was the other half of that commit (cross-lane reductions moved from ds_bpermute to DPP / v_permlane*_swap, the V^T staging rewrite).
# The flag stays for a measured reason of its own: beside MFMAs a v_pk_fma_f32 costs more issue time than the two v_fma_f32 it replaces
# (/opt/skills/guides/MI355X_MICROARCH.md, "price of one filler beside MFMAs": +22..26 cycles per pair) and hipcc SLP-packs the fp32
# epilogues of every MFMA kernel here.  Correctness does not depend on it; check_no_packed_fp32() only reports.
# The host pass of hipcc does not know the feature and says so; that warning is filtered below.
DEVICE_FLAGS = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
_HOST_NOISE = "is not a recognized feature for this target"


def _newer(a, b):
    return not os.path.exists(b) or os.path.getmtime(a) > os.path.getmtime(b)


def count_device_instructions(pattern, lib=LIB):
    """Disassemble the device code of the linked library and count the instructions matching the regular expression `pattern`.  None when
    llvm-objdump is not available."""
    import re
    import shutil
    import tempfile
    objdump = os.path.join(os.path.dirname(os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))), "..", "lib", "llvm", "bin", "llvm-objdump")
    if not os.path.exists(objdump):
        objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        return None
    tmp = tempfile.mkdtemp(prefix="cfen_disasm_")
    try:
        so = shutil.copy(lib, os.path.join(tmp, "lib.so"))
        subprocess.run([objdump, "--offloading", so], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=False)   # extracts the bundles beside it
        n = 0
        for f in sorted(os.listdir(tmp)):
            if "amdgcn" in f:
                out = subprocess.run([objdump, "-d", os.path.join(tmp, f)], capture_output=True, text=True, check=False).stdout
                n += len(re.findall(pattern, out))
        return n
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def check_no_packed_fp32(lib=LIB):
    """count v_pk_{fma,mul,add}_f32 in the linked library (see DEVICE_FLAGS: a performance choice, CFEN_CXXFLAGS or another hipcc could silently
    undo it).  Returns the number of such instructions (0 = as intended), None when llvm-objdump is not available."""
    return count_device_instructions(r"\bv_pk_(?:fma|mul|add)_f32\b", lib)


def check_no_ashr_pk_u8(lib=LIB):
    """count v_ashr_pk_u8_i32 in the linked library.  Unlike the packed-fp32 count this one is about CORRECTNESS: hipcc (ROCm 7.2) fuses shift +
    clamp + packing of two bytes into this instruction and then ORs further bytes into the destination's upper half as if it were zero, and on
    the MI355X byte 2 of such a dword came out wrong (csrc/k_yuv.hip, yv_dot).  No kernel here needs the instruction and the
    shipped build holds none, so any occurrence -- the workaround undone by another compiler, or new code that packs bytes -- is reported by
    build() and fails tests/test_yuv_host.py.  Returns the count (0 = as intended), None when llvm-objdump is not available."""
    return count_device_instructions(r"\bv_ashr_pk_u8_i32\b", lib)


def build(force=False, verbose=False, packed_fp32=False, lib=None, objdir=None):
    """packed_fp32 / lib / objdir: A/B build of the same sources WITH packed-fp32 code generation into another library
    (tools/repro_pk_fma.py); the shipped build is build()."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    lib = lib or LIB
    objdir = objdir or os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    include = os.path.join(os.path.dirname(HERE), "include")
    headers += [os.path.join(include, f) for f in os.listdir(include) if f.endswith(".h")]
    headers.append(os.path.abspath(__file__))          # flags live here
    objs = []
    procs = []
    for src in SOURCES:
        path = os.path.join(CSRC, src)
        if not os.path.exists(path):
            continue
        obj = os.path.join(objdir, src.rsplit(".", 1)[0] + ".o")
        objs.append(obj)
        if force or _newer(path, obj) or any(_newer(h, obj) for h in headers):
            cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-x", "hip", "-c", path, "-o", obj,
                   "-Wall", "-Wno-unused-function"] + ([] if packed_fp32 else DEVICE_FLAGS) + EXTRA_FLAGS.get(src, []) + os.environ.get("CFEN_CXXFLAGS", "").split()
            if verbose:
                print(" ".join(cmd), flush=True)
            procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    failed = False
    for src, p in procs:
        out = "\n".join(l for l in p.communicate()[0].decode().splitlines() if _HOST_NOISE not in l)
        if p.returncode != 0:
            failed = True
            sys.stderr.write("---- %s ----\n%s\n" % (src, out))
        elif verbose and out.strip():
            print(out)
    if failed:
        raise RuntimeError("hipcc failed")
    if procs or not os.path.exists(lib):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
        if not packed_fp32:
            n = check_no_packed_fp32(lib)
            if n:
                sys.stderr.write("note: libcfen_hip.so contains %d packed-fp32 VALU instructions (DEVICE_FLAGS overridden?): slower beside "
                                 "MFMAs, results unaffected\n" % n)
        n = check_no_ashr_pk_u8(lib)
        if n:
            sys.stderr.write("WARNING: libcfen_hip.so contains %d v_ashr_pk_u8_i32 instructions: this compiler's byte packing around it gave wrong "
                             "bytes on the MI355X (csrc/k_yuv.hip, yv_dot); run the GPU tests before trusting uint8 outputs\n" % n)
    return lib


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
