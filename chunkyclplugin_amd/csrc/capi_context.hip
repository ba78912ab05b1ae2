// capi_context.hip — the device context of include/chunky_hip.h: version, device count and name, chunky_init, chunky_shutdown.
#include "capi_internal.hpp"

// 0.4: chunky_run_callbacks carries its size (an ABI change), chunky_group_peer_status, CHUNKY_OPT_BVH_CULL_BEHIND
// 0.5: chunky_group_transport / chunky_group_set_transport (the group's read-back exchange through RCCL, bound at run time)
// 0.6: albedo and normal images for denoisers: chunky_render_aov_passes / _read / _reset / _kernel_time / _kernel_info
//      also: projected cameras (CHUNKY_PROJ_PARALLEL .. CHUNKY_PROJ_STEREOGRAPHIC), chunky_camera_rays, chunky_selftest_camera_rays
//      also: their lens and the ODS types: chunky_render_set_lens, chunky_camera_rays_lens, CHUNKY_PROJ_ODS, CHUNKY_PROJ_ODS_STACKED
//      also: the À-Trous denoiser: chunky_denoise_default_params / _host / _frame / _exp, chunky_render_denoise / _denoise_kernel_time
//      (additions only, so the version string stays "0.6": hosts that check it for the AOV calls keep working)
extern "C" const char* chunky_version(void) { return "chunky-hip 0.6 gfx950"; }

extern "C" int chunky_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int chunky_device_name(int device, char* buf, int buf_len) {
    if (!buf || buf_len <= 0) return fail(CHUNKY_E_INVALID, "chunky_device_name: no buffer");
    hipDeviceProp_t prop;
    if (device < 0 || device >= chunky_device_count()) return fail(CHUNKY_E_NO_DEVICE, "no HIP device %d", device);
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    // (some boxes report an empty marketing name)
    snprintf(buf, buf_len, "%s (%s, %d CUs)", prop.name[0] ? prop.name : "AMD GPU", prop.gcnArchName, prop.multiProcessorCount);
    return CHUNKY_OK;
}

extern "C" int chunky_init(int device, chunky_ctx** out) {
    if (!out) return fail(CHUNKY_E_INVALID, "chunky_init: out is NULL");
    *out = nullptr;
    int n = chunky_device_count();
    if (n <= 0) return fail(CHUNKY_E_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    if (device < 0 || device >= n) return fail(CHUNKY_E_NO_DEVICE, "device %d out of range (0..%d)", device, n - 1);
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<chunky_ctx> c(new chunky_ctx);
    c->device = device;
    HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    char nm[256];
    if (chunky_device_name(device, nm, sizeof nm) == CHUNKY_OK) c->name = nm;
    *out = c.release();
    return CHUNKY_OK;
}

extern "C" int chunky_shutdown(chunky_ctx* ctx) {
    if (!ctx) return fail(CHUNKY_E_INVALID, "chunky_shutdown: NULL context");
    if (!ctx->members.empty()) {
        int rc = CHUNKY_OK;
        if (!ctx->comms.empty()) {  // (the members' streams are idle by the contract of shutdown: no render target is left)
            for (chunky_ctx* m : ctx->members) {
                (void)hipSetDevice(m->device);
                (void)hipStreamSynchronize(m->stream);
            }
            group_close_rccl(ctx, false);
        }
        for (chunky_ctx* m : ctx->members)
            if (int e = chunky_shutdown(m)) rc = e;
        delete ctx;
        return rc;
    }
    {
        std::lock_guard<std::recursive_mutex> g(ctx->mu);
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
        if (ctx->gamma_table) (void)hipFree(ctx->gamma_table);
        (void)hipStreamDestroy(ctx->stream);
    }
    delete ctx;
    return CHUNKY_OK;
}
