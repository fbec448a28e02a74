"""Build the gfx950 shared library (C-ABI of include/cuttlefish_hip.h) in-tree with hipcc.

hipcc cross-compiles --offload-arch=gfx950 without a GPU; the resulting
cuttlefish_amd/libcuttlefish_hip.so travels to the GPU box with the snapshot.
"""
from __future__ import annotations

import os
import shutil
import subprocess

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, "csrc")
LIB = os.path.join(PKG, "libcuttlefish_hip.so")

# -ffp-contract=off: the kernels spell fused ops as fmaf() so that every float
# operation matches the CPU oracle bit for bit.
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC",
               "-shared", "-Wall", "-Wno-unused-function"]
# Flags of single translation units.  bc7_encode.hip: without SLP packing.  The packed fp32 operations the vectoriser
# forms (v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32) issue in 4.6 cycles against 2 x 2.7 for their plain halves
# (profiles/levels_valu_rate.txt), yet without them this issue-bound kernel executes the same number of VALU
# instructions in 1.8 % fewer wave cycles: Normal 7.42 -> 7.27 ms, no level slower, same bytes (profiles/levels_bc7_ab.txt).
PER_FILE_FLAGS = {"bc7_encode.hip": ["-fno-slp-vectorize"]}


def _file_flags(src: str):
    return PER_FILE_FLAGS.get(os.path.basename(src), [])


def sources():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip"))


def _deps():
    d = [os.path.join(CSRC, f) for f in os.listdir(CSRC)]
    d.append(os.path.join(os.path.dirname(PKG), "include", "cuttlefish_hip.h"))
    return d


def _fingerprint() -> str:
    """SHA-256 over the build flags and the CONTENT of every dependency: modification times are
    not trusted (git checkout / stash restore files with arbitrary times, and a stale library on
    the GPU box silently measures old kernels)."""
    import hashlib
    h = hashlib.sha256((" ".join(HIPCC_FLAGS) + repr(sorted(PER_FILE_FLAGS.items()))).encode())
    for p in sorted(_deps()):
        if os.path.isfile(p):
            h.update(os.path.basename(p).encode())
            with open(p, "rb") as f:
                h.update(f.read())
    return h.hexdigest()


STAMP = LIB + ".srchash"


def is_stale() -> bool:
    if not os.path.exists(LIB) or not os.path.exists(STAMP):
        return True
    with open(STAMP) as f:
        return f.read().strip() != _fingerprint()


def hipcc_path():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _object_key(src: str) -> str:
    """Content hash of one translation unit: flags, the source, every header of csrc/ and the ABI header."""
    import hashlib
    h = hashlib.sha256(" ".join(HIPCC_FLAGS + _file_flags(src)).encode())
    deps = [src] + sorted(p for p in _deps() if p.endswith(".h"))
    for p in deps:
        h.update(os.path.basename(p).encode())
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def build(force: bool = False, verbose: bool = False) -> str:
    """One object per .hip file (compiled in parallel, reused while its content hash stands:
    changing one kernel recompiles one file), then one link."""
    if not force and not is_stale():
        return LIB
    from concurrent.futures import ThreadPoolExecutor
    objdir = os.path.join(PKG, "build")
    os.makedirs(objdir, exist_ok=True)
    cflags = [f for f in HIPCC_FLAGS if f != "-shared"]

    def compile_one(src):
        base = os.path.splitext(os.path.basename(src))[0]
        obj = os.path.join(objdir, base + ".o")
        stamp = obj + ".key"
        key = _object_key(src)
        if not force and os.path.exists(obj) and os.path.exists(stamp):
            with open(stamp) as f:
                if f.read().strip() == key:
                    return obj
        cmd = [hipcc_path()] + cflags + _file_flags(src) + ["-c", "-o", obj + ".tmp", src]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
        os.replace(obj + ".tmp", obj)
        with open(stamp, "w") as f:
            f.write(key + "\n")
        return obj

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        objs = list(ex.map(compile_one, sources()))
    # the link line comes from the same flag list as the compiles (arch and anything link-relevant stay in step)
    lflags = [f for f in HIPCC_FLAGS if f.startswith(("--offload-arch", "-fgpu-rdc", "-fsanitize")) or f in ("-shared", "-fPIC")]
    cmd = [hipcc_path()] + lflags + ["-o", LIB + ".tmp"] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    check_no_vector_spills(LIB + ".tmp")          # a spilling build never becomes the library
    os.replace(LIB + ".tmp", LIB)
    with open(STAMP, "w") as f:
        f.write(_fingerprint() + "\n")
    return LIB


LLVM_BIN = "/opt/rocm/lib/llvm/bin"
BLOCK_KERNELS = ("cfhip_bc7_encode_kernel", "cfhip_bc15_encode_kernel", "cfhip_bc6h_encode_kernel",
                 "cfhip_etc_encode_kernel", "cfhip_astc_encode_kernel",
                 # the decoders (csrc/decode.hip): every cfhip_decode_*_kernel, the fused SSE ones included
                 "cfhip_decode_block_kernel", "cfhip_decode_astc_kernel", "cfhip_decode_sse_block_kernel",
                 "cfhip_decode_sse_astc_kernel",
                 # the batched decoders (csrc/decode.hip, csrc/decode_batch.h)
                 "cfhip_decode_batch_kernel", "cfhip_decode_batch_astc_kernel",
                 # the per-image pixel ops (csrc/image_ops.hip)
                 "cfhip_image_ops_kernel",
                 # the quality metrics (csrc/compare.hip)
                 "cfhip_compare_block_kernel", "cfhip_compare_astc_kernel", "cfhip_compare_ssim_kernel",
                 "cfhip_compare_final_kernel",
                 # their batched forms (csrc/compare.hip, csrc/compare_batch.h)
                 "cfhip_compare_batch_block_kernel", "cfhip_compare_batch_astc_kernel",
                 "cfhip_compare_batch_ssim_kernel", "cfhip_compare_batch_final_kernel",
                 # PVRTC1 4 bpp (csrc/pvrtc.hip): the encoder's passes and the decoder
                 "cfhip_pvrtc_load_kernel", "cfhip_pvrtc_init_kernel", "cfhip_pvrtc_mod_kernel",
                 "cfhip_pvrtc_refine_kernel", "cfhip_pvrtc_pack_kernel", "cfhip_pvrtc_decode_kernel",
                 "cfhip_pvrtc_decode_sse_kernel",
                 # the standard formats back to texels (csrc/std_unpack.hip) and their Pass A (csrc/compare.hip)
                 "cfhip_std_unpack_kernel", "cfhip_std_compare_kernel",
                 # the rate-distortion pass over BC1-5 / BC7 payloads (csrc/rdo.hip)
                 "cfhip_rdo_kernel", "cfhip_rdo2d_kernel",
                 # the deflate-size estimator (csrc/lzsize.hip); the sort between them is rocprim's
                 "cfhip_lz_keys_kernel", "cfhip_lz_match_kernel", "cfhip_lz_parse_kernel", "cfhip_lz_cost_kernel",
                 "cfhip_lz_final_kernel",
                 # the zlib encoder behind it (csrc/deflate.hip)
                 "cfhip_deflate_parse_kernel", "cfhip_deflate_adler_kernel", "cfhip_deflate_codes_kernel",
                 "cfhip_deflate_lengths_kernel", "cfhip_deflate_offsets_kernel", "cfhip_deflate_emit_kernel",
                 "cfhip_deflate_final_kernel",
                 # indexed zlib streams back to bytes (csrc/inflate.hip), and the encoder's index
                 "cfhip_inflate_decode_kernel", "cfhip_inflate_resolve_kernel", "cfhip_inflate_pack_kernel",
                 "cfhip_inflate_fold_kernel", "cfhip_inflate_final_kernel", "cfhip_zindex_kernel",
                 # LZ4 frames, both ways (csrc/lz4.hip); the encoder's match stage lives in csrc/lzsize.hip
                 "cfhip_lz4_match_kernel", "cfhip_lz4_parse_kernel", "cfhip_lz4_plan_kernel", "cfhip_lz4_offsets_kernel",
                 "cfhip_lz4_emit_kernel", "cfhip_lz4_hash_kernel", "cfhip_lz4_final_kernel", "cfhip_lz4_chain_kernel",
                 "cfhip_lz4_block_kernel", "cfhip_lz4_dfinal_kernel",
                 # PNG files of images (csrc/png.hip): the 24 filter kernels (source type x channels x depth), crc, final
                 "cfhip_png_filter_kernel", "cfhip_png_crc_kernel", "cfhip_png_final_kernel",
                 # the mip post-pass (csrc/mip_post.hip): alpha coverage and normal renormalisation
                 "cfhip_mip_post_gather_kernel", "cfhip_mip_post_count_kernel", "cfhip_mip_post_decide_kernel",
                 "cfhip_mip_post_apply_kernel",
                 # alpha bleeding (csrc/alpha_bleed.hip): pass 0, a step of the flood, the last step fused with the fill
                 "cfhip_alpha_bleed_seed_kernel", "cfhip_alpha_bleed_step_kernel", "cfhip_alpha_bleed_fill_kernel",
                 # the signed distance field from alpha (csrc/alpha_sdf.hip): classes, row distances, columns, tiles
                 "cfhip_alpha_sdf_classify_kernel", "cfhip_alpha_sdf_row_kernel", "cfhip_alpha_sdf_column_kernel",
                 "cfhip_alpha_sdf_resolve_kernel",
                 # specular anti-aliasing (csrc/spec_aa.hip): five levels from texels, five more from a launch's moments
                 "cfhip_spec_aa_texel_kernel", "cfhip_spec_aa_moment_kernel",
                 # ambient occlusion from height maps (csrc/height_ao.hip): the height plane, the scan per halo class
                 "cfhip_height_ao_plane_kernel", "cfhip_height_ao_scan_kernel",
                 # environment maps (csrc/envmap.hip): panorama to cube, the GGX chain and its copy, the SH9 rows and sum
                 "cfhip_equirect_to_cube_kernel", "cfhip_cube_prefilter_kernel", "cfhip_cube_copy_kernel",
                 "cfhip_cube_sh9_rows_kernel", "cfhip_cube_sh9_final_kernel",
                 # the BRDF lookup table (with and without the sheen column) and the irradiance cube (csrc/envmap.hip)
                 "cfhip_brdf_lut_kernel", "cfhip_cube_irradiance_kernel")


def kernel_metadata(lib: str = LIB):
    """{kernel name: {scratch, vgpr, agpr, vgpr_spill, sgpr_spill, lds}} read from the gfx950 code objects inside the
    built library (llvm-objdump --offloading + llvm-readelf --notes); None when the ROCm LLVM tools are absent."""
    import re
    import tempfile
    objdump, readelf = os.path.join(LLVM_BIN, "llvm-objdump"), os.path.join(LLVM_BIN, "llvm-readelf")
    if not (os.path.exists(lib) and os.path.exists(objdump) and os.path.exists(readelf)):
        return None
    out = {}
    with tempfile.TemporaryDirectory() as d:
        cp = shutil.copy(lib, d)                       # llvm-objdump --offloading extracts next to its input
        subprocess.run([objdump, "--offloading", cp], cwd=d, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        for f in sorted(os.listdir(d)):
            if "amdgcn" not in f:
                continue
            assert f.endswith("gfx950"), f             # one target, no fat binary
            notes = subprocess.run([readelf, "--notes", os.path.join(d, f)], check=True, capture_output=True, text=True).stdout
            # one YAML list item per kernel ("  - .agpr_count: ..." opens it: the keys are sorted, .name comes later)
            for item in re.split(r"\n\s+- (?=\.agpr_count:|\.args:)", notes):
                name = re.search(r"\.name:\s+(\S+)", item)
                if not name or ".vgpr_count" not in item:
                    continue

                def g(k):
                    m = re.search(r"\.%s:\s+(\d+)" % k, item)
                    return int(m.group(1)) if m else None
                out[name.group(1)] = {"scratch": g("private_segment_fixed_size"), "vgpr": g("vgpr_count"), "agpr": g("agpr_count"),
                                      "vgpr_spill": g("vgpr_spill_count"), "sgpr_spill": g("sgpr_spill_count"),
                                      "lds": g("group_segment_fixed_size")}
    return out


def check_no_vector_spills(lib: str = LIB):
    """A correctness rule, not a performance one (round 5): these kernels read each other's lanes (DPP, ds_bpermute,
    v_readlane), and a vector register spilled inside divergent control flow saves the active lanes only -- a spilling
    ETC2 build returned wrong blocks.  On gfx950 the compiler can also park VGPRs in AGPRs without touching scratch, so
    scratch == 0 alone does not prove it: every block kernel must show vgpr_spill_count 0, agpr_count 0 and no scratch.
    Raises RuntimeError naming the offenders; silently passes where the LLVM tools are missing."""
    meta = kernel_metadata(lib)
    if meta is None:
        return
    bad = {k: v for k, v in meta.items() if any(s in k for s in BLOCK_KERNELS) and
           (v["scratch"] != 0 or (v["vgpr_spill"] or 0) != 0 or (v["agpr"] or 0) != 0)}
    if bad:
        raise RuntimeError("block kernels with spilled vector registers (wrong blocks under divergence): %r" % (bad,))


if __name__ == "__main__":
    print(build(force=True, verbose=True))
