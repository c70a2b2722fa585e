"""In-tree build of the native pieces (hipcc for gfx950, g++ for the host shim).

Everything lands next to the sources so the built ``.so`` files travel with the
repo snapshot to the GPU box (they are git-ignored, not gpurun-ignored).
"""
from __future__ import annotations

import os
import shutil
import subprocess
from pathlib import Path

PKG = Path(__file__).resolve().parent
ROOT = PKG.parent
CSRC = PKG / "csrc"
INCLUDE = ROOT / "include"

LIB_ENGINE = PKG / "libmi355rec.so"        # HIP kernels + C-ABI (include/mi355rec.h)
LIB_SHIM = PKG / "librecommender_shim.so"  # C++ Recommender/DataManager drop-in
BIN_CLI = PKG / "recommender"              # drop-in CLI (main.cpp equivalent)

HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
OFFLOAD_ARCH = "gfx950"

ENGINE_SOURCES = [CSRC / "mi355rec.hip", CSRC / "sharded.hip"]
# (embed*.h belong to the companion library, build_embed below: the engine includes none of them)
ENGINE_DEPS = (ENGINE_SOURCES + sorted(p for p in CSRC.glob("*.h") if not p.name.startswith("embed"))
               + [INCLUDE / "mi355rec.h", INCLUDE / "mi355rec_diag.h"])

# -ffp-contract=off: the parity contract is sequential multiply-then-add with no
# FMA contraction (Recommender.cu:264-269 compiled by the reference Makefile:9).
HIP_FLAGS = [
    f"--offload-arch={OFFLOAD_ARCH}", "-O3", "-std=c++17", "-ffp-contract=off",
    "-fPIC", "-shared", f"-I{INCLUDE}", f"-I{CSRC}", "-ldl",
]


def _stale(target: Path, deps) -> bool:
    if not target.exists():
        return True
    t = target.stat().st_mtime
    return any(Path(d).stat().st_mtime > t for d in deps if Path(d).exists())


def _run(cmd) -> None:
    proc = subprocess.run([str(c) for c in cmd], capture_output=True, text=True)
    if proc.returncode != 0:
        raise RuntimeError(
            "build command failed:\n  " + " ".join(str(c) for c in cmd) + "\n" + (proc.stdout + proc.stderr)[-6000:]
        )


LLVM_BIN = Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "lib" / "llvm" / "bin"
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def kernel_metadata(lib: Path = LIB_ENGINE) -> list:
    """Per-kernel figures (name, vgpr_count, sgpr_count, lds, scratch) of the gfx950 code objects inside a
    built library — read from the artefact that ships, not from a second compile: the .hip_fatbin section is
    split into its offload bundles, each is unbundled and its AMDGPU metadata note parsed."""
    import re
    import tempfile

    out = []
    with tempfile.TemporaryDirectory() as tmp:
        fat = Path(tmp) / "fat.bin"
        _run([LLVM_BIN / "llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", lib, Path(tmp) / "copy.so"])
        blob = fat.read_bytes()
        starts = [m.start() for m in re.finditer(re.escape(BUNDLE_MAGIC), blob)]
        for i, a in enumerate(starts):
            b = starts[i + 1] if i + 1 < len(starts) else len(blob)
            part, co = Path(tmp) / f"bundle{i}.bin", Path(tmp) / f"dev{i}.co"
            part.write_bytes(blob[a:b])
            _run([LLVM_BIN / "clang-offload-bundler", "--unbundle", "--type=o", f"--input={part}",
                  f"--targets=hipv4-amdgcn-amd-amdhsa--{OFFLOAD_ARCH}", f"--output={co}"])
            notes = subprocess.run([str(LLVM_BIN / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True,
                                   check=True).stdout
            # one "- .agpr_count: ..." block per kernel inside amdhsa.kernels
            for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
                def field(name, conv=int):
                    m = re.search(r"\." + name + r":\s*(\S+)", block)
                    return conv(m.group(1)) if m else None
                out.append({"name": field("name", str), "vgpr": field("vgpr_count"), "sgpr": field("sgpr_count"),
                            "lds": field("group_segment_fixed_size"), "scratch": field("private_segment_fixed_size")})
    return out


def handoff_sites(lib: Path = LIB_ENGINE) -> list:
    """Disassembles the gfx950 code objects inside a built library and returns, for every "barrier, then one thread
    counts the workgroup in" site (an s_barrier followed within a few instructions by a RETURNING global_atomic_add:
    the arrival of a cross-workgroup hand-off), whether an `s_waitcnt vmcnt(0)` stands before that
    barrier: [(kernel, has_vmcnt0)].  A workgroup-scope fence does not wait for a wave's global stores on gfx950
    (ADVICE r3): without the wait the count can reach memory before the write-through stores it announces."""
    import re
    import tempfile

    sites = []
    with tempfile.TemporaryDirectory() as tmp:
        fat = Path(tmp) / "fat.bin"
        _run([LLVM_BIN / "llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", lib, Path(tmp) / "copy.so"])
        blob = fat.read_bytes()
        starts = [m.start() for m in re.finditer(re.escape(BUNDLE_MAGIC), blob)]
        for i, a in enumerate(starts):
            b = starts[i + 1] if i + 1 < len(starts) else len(blob)
            part, co = Path(tmp) / f"bundle{i}.bin", Path(tmp) / f"dev{i}.co"
            part.write_bytes(blob[a:b])
            _run([LLVM_BIN / "clang-offload-bundler", "--unbundle", "--type=o", f"--input={part}",
                  f"--targets=hipv4-amdgcn-amd-amdhsa--{OFFLOAD_ARCH}", f"--output={co}"])
            text = subprocess.run([str(LLVM_BIN / "llvm-objdump"), "-d", "--no-show-raw-insn", str(co)],
                                  capture_output=True, text=True, check=True).stdout
            kernel, window = None, []
            for line in text.splitlines():
                m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
                if m:
                    kernel, window = m.group(1), []
                    continue
                ins = line.strip()
                if not ins or kernel is None:
                    continue
                window.append(ins)
                del window[:-80]
                if ins.startswith("global_atomic_add") and " sc0" in ins:   # a returning add: somebody wants to know its place
                    near = window[-64:-1]
                    if any(x.startswith("s_barrier") for x in near):
                        before = window[:-1]
                        last_bar = max(j for j, x in enumerate(before) if x.startswith("s_barrier"))
                        sites.append((kernel, any("vmcnt(0)" in x for x in before[max(0, last_bar - 40):last_bar])))
    return sites


def check_no_scratch(lib: Path = LIB_ENGINE, tolerate=()) -> int:
    """No kernel of the engine may reserve private (scratch) memory: a dispatch of such a kernel sets up
    scratch even when no instruction touches it (scan_half_multi_kernel did, for a dead 16-byte stack slot:
    VERDICT r3 item 3b).  Returns the number of kernels looked at.
    `tolerate` (never used for the product library): (name fragment, bytes) pairs a VARIANT build may stay within."""
    meta = kernel_metadata(lib)
    if not meta:
        raise RuntimeError(f"no gfx950 kernel found inside {lib}")
    def tolerated(k):
        return k["scratch"] is not None and any(frag in k["name"] and k["scratch"] <= limit for frag, limit in tolerate)
    bad = [k for k in meta if (k["scratch"] is None or k["scratch"] > 0) and not tolerated(k)]
    if bad:
        raise RuntimeError("kernels that reserve scratch memory:\n  " +
                           "\n  ".join(f'{k["scratch"]} B  {k["name"]}' for k in bad))
    return len(meta)


CPU_BACKEND_SRC = CSRC / "cpu_backend.cpp"
CPU_BACKEND_OBJ = PKG / "cpu_backend.o"
CPU_BACKEND_DEPS = [CPU_BACKEND_SRC, CSRC / "cpu_backend.h", CSRC / "filter_check.h", CSRC / "weights_check.h",
                    CSRC / "playlist_request.h", CSRC / "rowset.h", CSRC / "rows_update.h", CSRC / "candidates.h"]
# The CPU backend (hosts without a HIP device) is plain C++ + OpenMP, compiled by g++ with the reference's own fp
# behaviour (Makefile:9: -O3, no -march, no -ffast-math; -ffp-contract=off keeps multiply and add apart) and
# linked into the engine library.
CPU_BACKEND_FLAGS = ["-std=c++17", "-O3", "-fopenmp", "-ffp-contract=off", "-fPIC", f"-I{INCLUDE}", f"-I{CSRC}"]


def build_engine(force: bool = False) -> Path:
    """Compile the HIP engine for gfx950 (cross-compiles without a GPU)."""
    if force or _stale(LIB_ENGINE, ENGINE_DEPS + CPU_BACKEND_DEPS):
        _run(["g++", *CPU_BACKEND_FLAGS, "-c", CPU_BACKEND_SRC, "-o", CPU_BACKEND_OBJ])
        # (the object goes in through the linker: hipcc would take a bare .o behind .hip sources for HIP source)
        _run([HIPCC, *HIP_FLAGS, "-o", LIB_ENGINE, *ENGINE_SOURCES, f"-Wl,{CPU_BACKEND_OBJ}", "-lgomp"])
        try:
            check_no_scratch(LIB_ENGINE)
        except Exception:
            LIB_ENGINE.unlink(missing_ok=True)   # a library that fails the check does not ship
            raise
    return LIB_ENGINE


LIB_EXPERIMENTS = PKG / "libmi355rec_experiments.so"   # -DMI355REC_EXPERIMENTS: the A/B routes and environment knobs (tools/, tests)


def build_engine_variant(out: Path, defines, force: bool = False, tolerate=()) -> Path:
    """Another build of the engine library with extra -D flags (never the product library): the MI355REC_EXPERIMENTS build
    keeps the routes that were moved out of the product (the fp16 single-query scan, the 8-bit front end of the
    multi-query pass) compiling, scratch-free and — tests/test_gpu_experiments.py — right."""
    if force or _stale(out, ENGINE_DEPS + CPU_BACKEND_DEPS):
        if _stale(CPU_BACKEND_OBJ, CPU_BACKEND_DEPS):
            _run(["g++", *CPU_BACKEND_FLAGS, "-c", CPU_BACKEND_SRC, "-o", CPU_BACKEND_OBJ])
        _run([HIPCC, *HIP_FLAGS, *[f"-D{d}" for d in defines], "-o", out, *ENGINE_SOURCES, f"-Wl,{CPU_BACKEND_OBJ}", "-lgomp"])
        try:
            check_no_scratch(out, tolerate)
        except Exception:
            out.unlink(missing_ok=True)
            raise
    return out


# scan_half_multi_kernel sits exactly on its budget (128 VGPRs, SGPRs spilled to lanes of the last one): with the two
# 8-bit-front-end instantiations in the module the allocator places a few dwords of hm_exact_step on the stack — in THIS build
# only (8 B in the fp16 variant, 28 B in the 8-bit ones); the product library is held to zero by build_engine().
EXPERIMENTS_TOLERATE = (("scan_half_multi_kernel", 32),)


def build_experiments(force: bool = False) -> Path:
    return build_engine_variant(LIB_EXPERIMENTS, ["MI355REC_EXPERIMENTS"], force, EXPERIMENTS_TOLERATE)


# The product's sources and flags + -DMI355REC_TEST_HOOKS: mi355rec_debug_handoff (include/mi355rec_diag.h), which poisons
# device buffers on purpose, is compiled into THIS library only.  The define changes host code alone, so the device code is
# the product's (tests/test_kernel_metadata.py compares the kernels of the two libraries); tests/test_gpu_testhooks.py runs
# the tests that break the hand-offs against it in a child process.
LIB_TESTHOOKS = PKG / "libmi355rec_testhooks.so"


def build_testhooks(force: bool = False) -> Path:
    return build_engine_variant(LIB_TESTHOOKS, ["MI355REC_TEST_HOOKS"], force)


# EMBEDDING TABLES: the companion library (include/mi355rec_embed.h).  Its own kernels, the engine's HIP_FLAGS, linked against
# the product library beside it; the product library's device code is not touched by anything it adds.
LIB_EMBED = PKG / "libmi355rec_embed.so"
EMBED_CPU_SRC = CSRC / "embed_cpu.cpp"
EMBED_CPU_OBJ = PKG / "embed_cpu.o"
EMBED_DEPS = [CSRC / "embed.hip", CSRC / "embed.hip.h", CSRC / "embed_request.h", EMBED_CPU_SRC, CSRC / "core.hip.h", CSRC / "merge.hip.h",
              CSRC / "embed_device.hip.h", CSRC / "experiments.hip.h", CSRC / "playlist_request.h", INCLUDE / "mi355rec_embed.h", INCLUDE / "mi355rec_diag.h",
              INCLUDE / "mi355rec.h"]


def build_embed(force: bool = False) -> Path:
    """Compile libmi355rec_embed.so for gfx950; check_no_scratch applies to it exactly as to the product library."""
    build_engine(force)
    if force or _stale(LIB_EMBED, EMBED_DEPS + [LIB_ENGINE]):
        _run(["g++", *CPU_BACKEND_FLAGS, "-c", EMBED_CPU_SRC, "-o", EMBED_CPU_OBJ])
        _run([HIPCC, *HIP_FLAGS, "-o", LIB_EMBED, CSRC / "embed.hip", f"-Wl,{EMBED_CPU_OBJ}", "-lgomp",
              f"-L{PKG}", "-lmi355rec", "-Wl,-rpath,$ORIGIN"])
        try:
            check_no_scratch(LIB_EMBED)
        except Exception:
            LIB_EMBED.unlink(missing_ok=True)
            raise
    return LIB_EMBED


# USER BATCHES: the second companion library (include/mi355rec_embed_batch.h).  Its own scan kernel over the embedding
# libraries' shared helpers (embed.hip.h, embed_device.hip.h), the engine's HIP_FLAGS, linked against the product library.
LIB_EMBED_BATCH = PKG / "libmi355rec_embed_batch.so"
EMBED_BATCH_DEPS = [CSRC / "embed_batch.hip", CSRC / "embed_batch.hip.h", CSRC / "embed_batch_request.h", CSRC / "embed.hip.h",
                    CSRC / "embed_device.hip.h",
                    CSRC / "embed_request.h", CSRC / "core.hip.h", CSRC / "merge.hip.h", CSRC / "experiments.hip.h", CSRC / "playlist_request.h",
                    INCLUDE / "mi355rec_embed_batch.h", INCLUDE / "mi355rec_embed.h", INCLUDE / "mi355rec_diag.h", INCLUDE / "mi355rec.h"]


def build_embed_batch(force: bool = False, pass_users: int = 0) -> Path:
    """Compile libmi355rec_embed_batch.so for gfx950; check_no_scratch applies to it exactly as to the product library.
    pass_users (2, 4 or 8; tools/run_embed_batch.py): a VARIANT beside it, libmi355rec_embed_batch_p<P>.so, whose passes take
    P users at every dim — what the per-dim choice of the product build is measured from."""
    build_engine(force)
    out = PKG / f"libmi355rec_embed_batch_p{pass_users}.so" if pass_users else LIB_EMBED_BATCH
    defines = [f"-DMI355REC_EMBED_BATCH_PASS_USERS={int(pass_users)}"] if pass_users else []
    if force or _stale(out, EMBED_BATCH_DEPS + [LIB_ENGINE]):
        _run([HIPCC, *HIP_FLAGS, *defines, "-o", out, CSRC / "embed_batch.hip", f"-L{PKG}", "-lmi355rec", "-Wl,-rpath,$ORIGIN"])
        try:
            check_no_scratch(out)
        except Exception:
            out.unlink(missing_ok=True)
            raise
    return out


# HALF-PRECISION EMBEDDING TABLES: the third companion library (include/mi355rec_embed_half.h).  Its row layout under the
# one scan body and host path of the embedding libraries (embed.hip.h, embed_device.hip.h), the engine's HIP_FLAGS, linked
# against the product library and against neither companion.
LIB_EMBED_HALF = PKG / "libmi355rec_embed_half.so"
EMBED_HALF_DEPS = [CSRC / "embed_half.hip", CSRC / "embed_half.hip.h", CSRC / "embed_half_request.h", CSRC / "embed.hip.h",
                   CSRC / "embed_device.hip.h",
                   CSRC / "embed_request.h", CSRC / "core.hip.h", CSRC / "merge.hip.h", CSRC / "experiments.hip.h", CSRC / "playlist_request.h",
                   INCLUDE / "mi355rec_embed_half.h", INCLUDE / "mi355rec_embed.h", INCLUDE / "mi355rec_diag.h", INCLUDE / "mi355rec.h"]


def build_embed_half(force: bool = False) -> Path:
    """Compile libmi355rec_embed_half.so for gfx950; check_no_scratch applies to it exactly as to the product library."""
    build_engine(force)
    if force or _stale(LIB_EMBED_HALF, EMBED_HALF_DEPS + [LIB_ENGINE]):
        _run([HIPCC, *HIP_FLAGS, "-o", LIB_EMBED_HALF, CSRC / "embed_half.hip", f"-L{PKG}", "-lmi355rec", "-Wl,-rpath,$ORIGIN"])
        try:
            check_no_scratch(LIB_EMBED_HALF)
        except Exception:
            LIB_EMBED_HALF.unlink(missing_ok=True)
            raise
    return LIB_EMBED_HALF


# RESTRICTED EMBEDDING REQUESTS: the fourth companion library (include/mi355rec_embed_sets.h).  The one scan body under a
# restriction policy, its own bitmaps and the embedding libraries' host path, the engine's HIP_FLAGS, linked against the
# product library and against no other companion.
LIB_EMBED_SETS = PKG / "libmi355rec_embed_sets.so"
EMBED_SETS_DEPS = [CSRC / "embed_sets.hip", CSRC / "embed_sets.hip.h", CSRC / "embed_sets_request.h", CSRC / "embed_half.hip.h",
                   CSRC / "embed_half_request.h", CSRC / "embed.hip.h", CSRC / "embed_device.hip.h",
                   CSRC / "embed_request.h", CSRC / "core.hip.h", CSRC / "merge.hip.h", CSRC / "experiments.hip.h", CSRC / "playlist_request.h",
                   INCLUDE / "mi355rec_embed_sets.h", INCLUDE / "mi355rec_embed_half.h", INCLUDE / "mi355rec_embed.h", INCLUDE / "mi355rec_diag.h",
                   INCLUDE / "mi355rec.h"]


def build_embed_sets(force: bool = False) -> Path:
    """Compile libmi355rec_embed_sets.so for gfx950; check_no_scratch applies to it exactly as to the product library."""
    build_engine(force)
    if force or _stale(LIB_EMBED_SETS, EMBED_SETS_DEPS + [LIB_ENGINE]):
        _run([HIPCC, *HIP_FLAGS, "-o", LIB_EMBED_SETS, CSRC / "embed_sets.hip", f"-L{PKG}", "-lmi355rec", "-Wl,-rpath,$ORIGIN"])
        try:
            check_no_scratch(LIB_EMBED_SETS)
        except Exception:
            LIB_EMBED_SETS.unlink(missing_ok=True)
            raise
    return LIB_EMBED_SETS


# STREAMED EMBEDDING REQUESTS: the fifth companion library (include/mi355rec_embed_stream.h).  The scan bodies of the
# embedding libraries and merge_kernel, instantiated here, its own prepare and finish kernels (embed_stream.hip.h), the
# engine's HIP_FLAGS, linked against the product library and against no other companion.
LIB_EMBED_STREAM = PKG / "libmi355rec_embed_stream.so"
EMBED_STREAM_DEPS = [CSRC / "embed_stream.hip", CSRC / "embed_stream.hip.h", CSRC / "embed_stream_request.h", CSRC / "embed_batch.hip.h",
                     CSRC / "embed_half.hip.h", CSRC / "embed_half_request.h", CSRC / "embed.hip.h", CSRC / "embed_device.hip.h",
                     CSRC / "embed_request.h", CSRC / "core.hip.h", CSRC / "merge.hip.h", CSRC / "experiments.hip.h", CSRC / "playlist_request.h",
                     INCLUDE / "mi355rec_embed_stream.h", INCLUDE / "mi355rec_embed_half.h", INCLUDE / "mi355rec_embed.h", INCLUDE / "mi355rec_diag.h",
                     INCLUDE / "mi355rec.h"]


def build_embed_stream(force: bool = False) -> Path:
    """Compile libmi355rec_embed_stream.so for gfx950; check_no_scratch applies to it exactly as to the product library."""
    build_engine(force)
    if force or _stale(LIB_EMBED_STREAM, EMBED_STREAM_DEPS + [LIB_ENGINE]):
        _run([HIPCC, *HIP_FLAGS, "-o", LIB_EMBED_STREAM, CSRC / "embed_stream.hip", f"-L{PKG}", "-lmi355rec", "-Wl,-rpath,$ORIGIN"])
        try:
            check_no_scratch(LIB_EMBED_STREAM)
        except Exception:
            LIB_EMBED_STREAM.unlink(missing_ok=True)
            raise
    return LIB_EMBED_STREAM


# EMBEDDING CANDIDATE LISTS: the sixth companion library (include/mi355rec_embed_cand.h).  Its own gather and claim kernels
# (embed_cand.hip.h) over the row layouts of the embedding libraries, the stream library's prepare and finish kernels and
# merge_kernel, instantiated here, the engine's HIP_FLAGS, linked against the product library and against no other companion.
LIB_EMBED_CAND = PKG / "libmi355rec_embed_cand.so"
EMBED_CAND_DEPS = ([CSRC / "embed_cand.hip", CSRC / "embed_cand.hip.h", CSRC / "embed_cand_request.h", INCLUDE / "mi355rec_embed_cand.h"]
                   + [d for d in EMBED_STREAM_DEPS if d.name != "embed_stream.hip"])   # (every header of the stream library is included)


def build_embed_cand(force: bool = False) -> Path:
    """Compile libmi355rec_embed_cand.so for gfx950; check_no_scratch applies to it exactly as to the product library."""
    build_engine(force)
    if force or _stale(LIB_EMBED_CAND, EMBED_CAND_DEPS + [LIB_ENGINE]):
        _run([HIPCC, *HIP_FLAGS, "-o", LIB_EMBED_CAND, CSRC / "embed_cand.hip", f"-L{PKG}", "-lmi355rec", "-Wl,-rpath,$ORIGIN"])
        try:
            check_no_scratch(LIB_EMBED_CAND)
        except Exception:
            LIB_EMBED_CAND.unlink(missing_ok=True)
            raise
    return LIB_EMBED_CAND


# MULTI-INTEREST EMBEDDING REQUESTS: the seventh companion library (include/mi355rec_embed_multi.h).  Its own scan and finish
# kernels (embed_multi.hip.h) over the row layouts of the embedding libraries, the stream library's prepare kernel and
# merge_kernel, instantiated here, the engine's HIP_FLAGS, linked against the product library and against no other companion.
LIB_EMBED_MULTI = PKG / "libmi355rec_embed_multi.so"
EMBED_MULTI_DEPS = ([CSRC / "embed_multi.hip", CSRC / "embed_multi.hip.h", CSRC / "embed_multi_request.h", INCLUDE / "mi355rec_embed_multi.h"]
                    + [d for d in EMBED_STREAM_DEPS if d.name != "embed_stream.hip"])   # (every header of the stream library is included)


def build_embed_multi(force: bool = False) -> Path:
    """Compile libmi355rec_embed_multi.so for gfx950; check_no_scratch applies to it exactly as to the product library."""
    build_engine(force)
    if force or _stale(LIB_EMBED_MULTI, EMBED_MULTI_DEPS + [LIB_ENGINE]):
        _run([HIPCC, *HIP_FLAGS, "-o", LIB_EMBED_MULTI, CSRC / "embed_multi.hip", f"-L{PKG}", "-lmi355rec", "-Wl,-rpath,$ORIGIN"])
        try:
            check_no_scratch(LIB_EMBED_MULTI)
        except Exception:
            LIB_EMBED_MULTI.unlink(missing_ok=True)
            raise
    return LIB_EMBED_MULTI


def shim_sources():
    return [CSRC / "Recommender.cpp", CSRC / "DataManager.cpp"]


def build_shim(force: bool = False) -> Path:
    """Compile the C++ drop-in (Recommender/DataManager over the C-ABI) and CLI."""
    srcs = [s for s in shim_sources() if s.exists()]
    if not srcs:
        return LIB_SHIM
    deps = srcs + [INCLUDE / "Recommender.h", INCLUDE / "Song.h", INCLUDE / "DataManager.h",
                   INCLUDE / "mi355rec.h", INCLUDE / "mi355rec_diag.h"]
    build_engine(force)
    common = ["g++", "-std=c++17", "-O2", "-fPIC", "-ffp-contract=off", f"-I{INCLUDE}"]
    link = [f"-L{PKG}", "-lmi355rec", "-Wl,-rpath,$ORIGIN"]
    if force or _stale(LIB_SHIM, deps + [CSRC / "shim_capi.cpp", LIB_ENGINE]):
        _run([*common, "-shared", "-o", LIB_SHIM, *srcs, CSRC / "shim_capi.cpp", *link])
    main_cpp = CSRC / "main.cpp"
    if main_cpp.exists() and (force or _stale(BIN_CLI, deps + [main_cpp, LIB_SHIM])):
        _run([*common, "-o", BIN_CLI, main_cpp, *srcs, *link])
    return LIB_SHIM


def build_oracle(force: bool = False) -> Path:
    """Build the CPU oracle (test infrastructure; see oracle/README.md)."""
    odir = ROOT / "oracle"
    target = odir / "liboracle.so"
    if force or _stale(target, [odir / "cosine_oracle.c", odir / "cosine_oracle.h"]):
        _run(["make", "-C", odir, "liboracle.so"])
    # (the Makefile's `ref` target builds oracle/_ref only where the reference tree is present AND readable by the user
    # building: a tree this user may not read counts as absent, whatever was prebuilt is kept)
    ref = odir / "_ref" / "libref_dm.so"
    if force or _stale(ref, [odir / "ref_dm_driver.cpp"]):
        _run(["make", "-C", odir, "ref"])
    return target


def build_all(force: bool = False) -> None:
    build_engine(force)
    build_experiments(force)   # (a second library; nothing in the product loads it)
    build_testhooks(force)     # (a third: the product + the test hooks, for tests/ only)
    build_embed(force)         # (the companion library: embedding tables over the product's C-ABI)
    build_embed_batch(force)   # (the second companion: user batches over an embedding table)
    build_embed_half(force)    # (the third companion: fp16 / bf16 embedding tables)
    build_embed_sets(force)    # (the fourth companion: hybrid requests restricted by row sets)
    build_embed_stream(force)  # (the fifth companion: device tensors in and out on the caller's stream)
    build_embed_cand(force)    # (the sixth companion: rank or score the listed rows of an embedding table by gather)
    build_embed_multi(force)   # (the seventh companion: one pass for the K interests of one user, with attribution)
    build_shim(force)
    build_oracle(force)


if __name__ == "__main__":
    build_all(force=True)
    print("built:", LIB_ENGINE)
