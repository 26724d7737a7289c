// Launchers of layer_taps.hip: the tap points of the layer-wise confidence branch (rgqa_config.conf_branch = 2)
#pragma once
#define TAP_MAX_LAYERS 12        // = GEMM_NT_MAX_PROBLEMS: the X projector GEMMs are the problems of one grouped launch
// p[i]: language output of cross-modality layer i (what get_activation("x<i>_lang") serves); compact[i] != 0: its rows are the B [CLS] rows already
struct TapSrcs { const void* p[TAP_MAX_LAYERS]; int compact[TAP_MAX_LAYERS]; };
// dst [X, B, row_bytes] <- row(b) of every source, bytes unchanged; row(b) = compact ? b : (cu ? cu[b] : b * stride_rows).  img (split-f32 rows only, else null):
// the rows' bf16 image [X, B, row_bytes / 2]
int k_tap_gather(const TapSrcs& srcs, int X, int B, const int* cu, int stride_rows, int row_bytes, void* dst, void* img, hipStream_t s);
// dy[row(b)][0 .. cols) += dtap[b][0 .. cols) for b < B, added in f32 and rounded once to T; row(b) = cu ? cu[b] : b * stride_rows
template <typename T> int k_tap_inject(const T* dtap, int ldt, T* dy, int ldy, const int* cu, int stride_rows, int B, int cols, hipStream_t s);
