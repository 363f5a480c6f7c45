#include "common.h"
#include "../../include/vfn_hip.h"
// 2: vfn_conv_desc.w_packed, vfn_bankscan_desc.precision, vfn_memread_desc.precision; bf16 / bf16x3 and I/O entry points
// 3: vfn_memread_desc.wide (added at 2 without a bump), vfn_conv_cfg_info, vfn_sizeof_desc
// 4: PNG / JPEG / segment-uncertainty / norm-refresh entry points (round 2)
// 13: vfn_bankmatch_desc, vfn_bank_match_certified, vfn_bank_refresh_lp_keys
// 15: vfn_conv_cfg_modes
// 16: vfn_train_aug_desc, vfn_train_aug_* (training clips)
// 18: vfn_imgseg_*, vfn_ln_colsum_batch_f32, vfn_ln_se_gate_batch_f32, vfn_ln_scale_rows_f32 (image segmentation on the device)
extern "C" int vfn_abi_version(void) { return VFN_ABI_VERSION; }

// sizeof of every descriptor as THIS library was compiled: a binding that read another header than this library's
// (v-floodnet_amd/_lib.py derives its structs from include/vfn_hip.h) fails its load-time check instead of
// reading past the caller's struct
extern "C" int vfn_sizeof_desc(int which) {
    switch (which) {
        case VFN_DESC_CONV: return (int)sizeof(vfn_conv_desc);
        case VFN_DESC_STEM: return (int)sizeof(vfn_stem_desc);
        case VFN_DESC_BANKSCAN: return (int)sizeof(vfn_bankscan_desc);
        case VFN_DESC_MEMREAD: return (int)sizeof(vfn_memread_desc);
        case VFN_DESC_BANK: return (int)sizeof(vfn_bank_desc);
        case VFN_DESC_WGRAD: return (int)sizeof(vfn_wgrad_desc);
        case VFN_DESC_REFRESH_FILTER: return (int)sizeof(vfn_refresh_filter);
        case VFN_DESC_REFRESH_EPILOGUE: return (int)sizeof(vfn_refresh_epilogue);
        case VFN_DESC_GATHER: return (int)sizeof(vfn_gather_entry);
        case VFN_DESC_BANKMATCH: return (int)sizeof(vfn_bankmatch_desc);
        case VFN_DESC_TRAIN_AUG: return (int)sizeof(vfn_train_aug_desc);
    }
    return -1;
}
