// C ABI of the PNG entries (bnhip_png_max_bytes, bnhip_png_workspace_size, bnhip_png_encode_device, bnhip_png_encode_u8).  The entry
// that renders and encodes in one call, bnhip_spectrogram_png_pcm16, is in api_spectrogram.cpp beside the render's tables.
#include <hip/hip_runtime.h>

#include "api_oneshot.h"
#include "png.h"

namespace bnhip {

int png_args_check(int n_images, int width, int height) {
    if (n_images < 1 || n_images > 65535) return set_err(BNHIP_E_INVALID, "n_images must be in [1, 65535]");
    if (width < 1 || width > PNG_MAX_DIM) return set_err(BNHIP_E_INVALID, "width must be in [1, 4096]");
    if (height < 1 || height > PNG_MAX_DIM) return set_err(BNHIP_E_INVALID, "height must be in [1, 4096]");
    return 0;
}

int png_cap_check(int n_images, int width, int height, size_t out_cap) {
    if (out_cap < png_max_bytes(n_images, width, height)) return set_err(BNHIP_E_INVALID, "out_cap smaller than bnhip_png_max_bytes");
    return 0;
}

}  // namespace bnhip

using namespace bnhip;

extern "C" {

int bnhip_png_max_bytes(int n_images, int width, int height, size_t* bytes) {
    if (!bytes) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    const int rc = png_args_check(n_images, width, height);
    if (rc) return rc;
    *bytes = png_max_bytes(n_images, width, height);
    return BNHIP_OK;
}

int bnhip_png_workspace_size(int n_images, int width, int height, size_t* bytes) {
    if (!bytes) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    const int rc = png_args_check(n_images, width, height);
    if (rc) return rc;
    *bytes = png_workspace_bytes(n_images, width, height);
    return BNHIP_OK;
}

int bnhip_png_encode_device(int device, const uint8_t* d_images, int n_images, int width, int height, const uint8_t* palette, uint8_t* d_out,
                            size_t out_cap, uint64_t* d_offsets, void* d_workspace, size_t workspace_bytes, void* hip_stream) {
    if (!d_images || !palette || !d_out || !d_offsets || !d_workspace) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    int rc = png_args_check(n_images, width, height);
    if (!rc) rc = png_cap_check(n_images, width, height, out_cap);
    if (!rc) rc = workspace_check(d_workspace, workspace_bytes, png_workspace_bytes(n_images, width, height), "bnhip_png_workspace_size");
    if (!rc) rc = use_device(device);
    if (rc) return rc;
    launch_png(d_images, png_work(n_images, width, height, palette, d_workspace), d_out, out_cap, (unsigned long long*)d_offsets,
               reinterpret_cast<hipStream_t>(hip_stream));
    return launch_status("png_encode_device");
    BN_GUARD_END((void)0)
}

int bnhip_png_encode_u8(int device, const uint8_t* images, int n_images, int width, int height, const uint8_t* palette, uint8_t* out,
                        size_t out_cap, uint64_t* offsets) {
    if (!images || !palette || !out || !offsets) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    int rc = png_args_check(n_images, width, height);
    if (!rc) rc = png_cap_check(n_images, width, height, out_cap);
    if (!rc) rc = use_device(device);
    if (rc) return rc;
    // one DevCarve: the images, the streams, the offsets, the workspace
    const size_t img_bytes = (size_t)n_images * height * width, cap = png_max_bytes(n_images, width, height);
    DevCarve cv;
    const size_t o_img = cv.add(img_bytes), o_bytes = cv.add(cap), o_off = cv.add(((size_t)n_images + 1) * 8);
    const size_t o_ws = cv.add(png_workspace_bytes(n_images, width, height));
    DevBlocks b;
    cv.alloc(b);
    uint8_t *d_img = cv.at<uint8_t>(o_img), *d_bytes = cv.at<uint8_t>(o_bytes);
    unsigned long long* d_offsets = cv.at<unsigned long long>(o_off);
    if (b.he == hipSuccess) b.he = hipMemcpy(d_img, images, img_bytes, hipMemcpyHostToDevice);
    if (b.he == hipSuccess) {
        launch_png(d_img, png_work(n_images, width, height, palette, cv.at<void>(o_ws)), d_bytes, cap, d_offsets, nullptr);
        b.he = hipGetLastError();
    }
    if (b.he == hipSuccess) b.he = fetch_streams(d_offsets, d_bytes, n_images, offsets, out);
    return b.he == hipSuccess ? BNHIP_OK : hip_fail("png_encode_u8", b);
    BN_GUARD_END((void)0)
}

}  // extern "C"
