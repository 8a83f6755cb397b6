// step_kernels.hip -- the kernels of the step by name: every unit lists its own (common.hpp: StepKernel), here they are one list, and
// what the runtime says of one of them is read from the loaded code object (the residency rule is checked against it).
#include "common.hpp"

using namespace mdbg;

static const StepKernel *step_kernel_at(uint32_t i) {
    const StepKernel *(*const tables[])(uint32_t *) = {scan_step_kernels, minimizers_step_kernels, prims_step_kernels, partition_step_kernels, extract_step_kernels, stitch_step_kernels, mapper_step_kernels, select_step_kernels, verify_step_kernels, realign_step_kernels};
    for (auto table : tables) {
        uint32_t n = 0;
        const StepKernel *k = table(&n);
        if (i < n) return k + i;
        i -= n;
    }
    return nullptr;
}

extern "C" const char *mdbg_step_kernel_name(uint32_t index) {
    const StepKernel *k = step_kernel_at(index);
    return k ? k->name : nullptr;
}

extern "C" int mdbg_kernel_attributes(mdbg_ctx *ctx, const char *kernel, uint64_t attr[8]) try {
    if (!ctx || !kernel || !attr) return set_error(ctx, MDBG_EINVAL, "mdbg_kernel_attributes: null argument");
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    for (uint32_t i = 0;; i++) {
        const StepKernel *k = step_kernel_at(i);
        if (!k) return set_error(ctx, MDBG_EINVAL, "mdbg_kernel_attributes: no kernel '%s'", kernel);
        if (strcmp(k->name, kernel) != 0) continue;
        hipFuncAttributes at;
        MDBG_HIP_CHECK(ctx, hipFuncGetAttributes(&at, k->fn));
        attr[0] = (uint64_t)at.numRegs; attr[1] = at.sharedSizeBytes; attr[2] = (uint64_t)at.maxThreadsPerBlock; attr[3] = k->threads;
        attr[4] = k->role; attr[5] = at.localSizeBytes; attr[6] = 0; attr[7] = 0;
        return MDBG_OK;
    }
} MDBG_API_CATCH(ctx)
