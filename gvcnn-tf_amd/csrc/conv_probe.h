// The probe bits of the convolution family: what gv_conv2d_set_debug(bits) switches.  The hook's value is copied into
// ConvArgs::dbg and ConvStats::dbg of every launch (conv_igemm.hip), so one number reaches every kernel at once.
// Three kinds:
//   SELECT    another CORRECT product path (a launcher's choice, or a kernel-uniform branch): outputs stay right, tests
//             may use it (the Python side names the two that tests use: _lib.PROBE_TAP_MAJOR, PROBE_GENERAL_EPILOGUE);
//   A/B       a scheduling or addressing variant inside a kernel: same values, for timing one against the other;
//   ABLATION  part of the work is skipped: the product library then computes GARBAGE (or nothing).  Timing tools only
//             (tools/ws_phase_times.py, tools/ws_ablate.sh and their like), never tests.
// The numbers are recorded in tools/ and in the committed profiles and do not change.  A number that means two things
// has two names of the same value; setting it switches both.
#pragma once

namespace gvconv {

enum Probe : int {
    // SELECT: lp_epilogue_lean_ok (conv_common.h) says no — every 16-bit launch takes the full staged epilogue
    PROBE_FULL_EPILOGUE = 2,
    // ABLATION: no epilogue stores, the accumulators kept live (conv_epilogue, x3_epilogue_staged, lp_epilogue_staged;
    // conv_ws then also leaves its fast epilogue for the general one, which stores nothing)
    PROBE_NO_STORES = 4,
    // ABLATION, conv_igemm_bf16s (conv_bf16s.hip): no plane split, wrong values
    PROBE_NO_SPLIT = 8,
    // ABLATION, conv_igemm_bf16s: no A loads
    PROBE_NO_A_LOADS = 16,
    // ABLATION, conv_igemm_bf16s: no LDS writes (operands stay live)
    PROBE_NO_LDS_WRITES = 32,
    // SELECT, conv_dma.hip three-plane launcher: an fp32 destination takes the direct epilogue, not the staged one
    PROBE_X3_DIRECT_EPILOGUE = 64,
    // SELECT, conv_dma.hip launcher: k-tiles tap-major (korder 0) where channel-chunk-major would be taken
    PROBE_TAP_MAJOR = 128,
    // A/B, conv_dma: no raised priority for waves 4-7 and every wave takes the k-tile barrier in front
    PROBE_DMA_NO_PHASING = 256,
    // A/B, conv_dma / conv_lp / conv_ws: the epilogue's per-column constants from global memory, not the LDS table
    PROBE_SS_FROM_GLOBAL = 512,
    // SELECT, conv_lp.hip halo launcher: one output row per wave where two would be taken
    PROBE_HALO_ONE_ROW = 1024,
    // ABLATION, conv_stats.h stat_publish: the BatchNorm sums never leave the workgroup
    PROBE_STAT_NO_PUBLISH = 2048,
    // 4096 — A/B, conv_ws loaders: no s_setprio;  ABLATION, conv_stats.h: no additions to the sums table
    PROBE_WS_NO_PRIO = 4096,
    PROBE_STAT_NO_TABLE = 4096,
    // 8192 — A/B, conv_ws consumers: waves NC/2.. take each barrier half a k-step later (the stagger; off by default);
    // ABLATION, conv_lp.hip / conv_lp_epi.h: no BatchNorm sums of the stored values
    PROBE_WS_STAGGER = 8192,
    PROBE_STAT_NO_SUMS = 8192,
    // 16384 — ABLATION, conv_ws / conv_ws_x3: the consumers alone, no loader work and no k-loop barriers;
    // ABLATION, conv_lp / conv_dma: no table initialisation and no barrier around the BatchNorm sums table
    PROBE_WS_CONSUMERS_ALONE = 16384,
    PROBE_STAT_NO_BARRIER = 16384,
    // ABLATION, conv_ws / conv_ws_x3 loaders: barriers but no loads
    PROBE_WS_NO_LOADS = 32768,
    // ABLATION, conv_ws / conv_ws_x3: loads but no barriers anywhere in the k-loop
    PROBE_WS_NO_BARRIERS = 65536,
    // SELECT, conv_ws: the general staged epilogue where the pipelined fast one would be taken
    PROBE_GENERAL_EPILOGUE = 1048576,
    // RETIRED, not to be reused: 8 in launch_halo_x3 (the 32x32x16 wide-strip form of conv3x3_halo_x3, superseded by
    // conv3x3_halo_x3_k32) and 4 / 16 / 32 there (its timing-only instantiations); 2097152 (the tap-table form of conv_ws,
    // measured neutral: profiles/r6_ws_diet_ab.txt)
};

}  // namespace gvconv
