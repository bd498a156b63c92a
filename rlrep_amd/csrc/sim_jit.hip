// Fused simulators of a kind compiled at run time (include/rlrep.h rlrep_sim_kind_*, rlrep_simx_*): the host side.  The text
// that is compiled is  sim_jit.h (carried in the library as a string: build.sh writes it into sim_jit_text.inc)  +  the user's struct  +
// static_asserts that hold the struct's constants to the description  +  RL_SIMX_KERNELS(name, jit).  hiprtc compiles it for the device's
// architecture with -O3 -ffp-contract=off; the code object is loaded with hipModuleLoadData and its three kernels are launched with
// hipModuleLaunchKernel -- one launch each, capturable, nothing allocated, synchronised or read on the host.  No kernel lives in this file.
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>
#include <algorithm>
#include <cctype>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/rlrep.h"
#include "common.h"
#include "kparams.h"
#include "launchers.h"
#include "sim_jit.h"

static const char k_simx_text[] =
#include "sim_jit_text.inc"
    ;

static_assert(sizeof(SimxState) == sizeof(rlrep_simx_state) && offsetof(SimxState, x) == offsetof(rlrep_simx_state, x) &&
              offsetof(SimxState, t) == offsetof(rlrep_simx_state, t) && offsetof(SimxState, obs) == offsetof(rlrep_simx_state, obs) &&
              offsetof(SimxState, n) == offsetof(rlrep_simx_state, n) && offsetof(SimxState, auto_restart) == offsetof(rlrep_simx_state, auto_restart) &&
              offsetof(SimxState, seed) == offsetof(rlrep_simx_state, seed), "include/rlrep.h rlrep_simx_state (sim_jit.h SimxState)");
static_assert(SIMX_CTL_CALLS == RL_CTL_CALLS && SIMX_CTL_T == RL_CTL_T && SIMX_CTL_ITER == RL_CTL_ITER && SIMX_CTL_START == RL_CTL_START &&
              SIMX_CTL_SIZE == RL_CTL_SIZE && SIMX_CTL_WARM == RL_CTL_WARM, "sim_jit.h restates the loop record (kparams.h RL_CTL_*)");

struct rlrep_sim_kind {
    rlrep_sim_kind_info_t info;        // FIRST (include/rlrep.h says so): what the launches' refusals read, and nothing else before the launch
    hipModule_t mod;
    hipFunction_t fn[3];               // start, step, step_append_ctl
};

// what the description itself must satisfy, by the entry point's name `who`
static bool desc_check(const char* who, const rlrep_sim_kind_desc* d) {
    if (!d) { rl_set_error("%s: bad argument (null description)", who); return false; }
    if (!d->source || !d->source[0]) { rl_set_error("%s: the kind's source text is null or empty", who); return false; }
    if (!d->name || !(isalpha((unsigned char)d->name[0]) || d->name[0] == '_')) { rl_set_error("%s: the kind's name must be the C identifier of its struct", who); return false; }
    for (const char* p = d->name; *p; ++p)
        if (!(isalnum((unsigned char)*p) || *p == '_') || p - d->name >= 128) { rl_set_error("%s: the kind's name must be the C identifier of its struct", who); return false; }
    if (d->S < 1 || d->S > RLREP_SIMX_MAX_S) { rl_set_error("%s: S %d outside [1, %d]", who, d->S, RLREP_SIMX_MAX_S); return false; }
    if (d->A < 1 || d->A > RLREP_SIMX_MAX_A) { rl_set_error("%s: A %d outside [1, %d]", who, d->A, RLREP_SIMX_MAX_A); return false; }
    if (d->NX < 1 || d->NX > RLREP_SIMX_MAX_NX) { rl_set_error("%s: NX %d outside [1, %d]", who, d->NX, RLREP_SIMX_MAX_NX); return false; }
    if (d->limit < 1) { rl_set_error("%s: limit %d below 1", who, d->limit); return false; }
    return true;
}

static std::string assemble(const rlrep_sim_kind_desc* d) {
    std::string t(k_simx_text);
    char tail[1024];
    t += "\n// ---- the kind ----\n#line 1 \"";
    t += d->name;
    t += "\"\n";
    t += d->source;
    snprintf(tail, sizeof(tail),
             "\n// ---- the description (rlrep_sim_kind_desc) ----\n"
             "static_assert(%s::S == %d, \"the struct's S differs from the description\");\n"
             "static_assert(%s::A == %d, \"the struct's A differs from the description\");\n"
             "static_assert(%s::NX == %d, \"the struct's NX differs from the description\");\n"
             "static_assert(%s::LIMIT == %d, \"the struct's LIMIT differs from the description\");\n"
             "static_assert(%s::TERMINATES == %s, \"the struct's TERMINATES differs from the description\");\n"
             "RL_SIMX_KERNELS(%s, jit)\n",
             d->name, d->S, d->name, d->A, d->name, d->NX, d->name, d->limit, d->name, d->terminates ? "true" : "false", d->name);
    t += tail;
    return t;
}

// the compiler's log from its first error on (the buffer of rlrep_last_error is short)
static void set_compile_error(const char* who, const char* what, const std::string& log) {
    size_t at = log.find("error");
    if (at == std::string::npos) at = 0;
    else { const size_t nl = log.rfind('\n', at); at = nl == std::string::npos ? 0 : nl + 1; }
    rl_set_error("%s: %s: %s", who, what, log.c_str() + at);
}

// text -> code object for `arch`; no device is touched
static int compile_code(const char* who, const rlrep_sim_kind_desc* d, const char* arch, std::vector<char>& code) {
    const std::string text = assemble(d);
    hiprtcProgram prog;
    hiprtcResult r = hiprtcCreateProgram(&prog, text.c_str(), "rlrep_sim_kind.hip", 0, nullptr, nullptr);
    if (r != HIPRTC_SUCCESS) { rl_set_error("%s: hiprtcCreateProgram: %s", who, hiprtcGetErrorString(r)); return RLREP_ERR_HIP; }
    const std::string archopt = std::string("--offload-arch=") + arch;
    const char* opts[] = {archopt.c_str(), "-O3", "-ffp-contract=off", "-std=c++17"};
    r = hiprtcCompileProgram(prog, 4, opts);
    if (r != HIPRTC_SUCCESS) {
        size_t n = 0;
        std::string log;
        if (hiprtcGetProgramLogSize(prog, &n) == HIPRTC_SUCCESS && n > 1) { log.resize(n); hiprtcGetProgramLog(prog, &log[0]); }
        set_compile_error(who, hiprtcGetErrorString(r), log);
        hiprtcDestroyProgram(&prog);
        return RLREP_ERR_HIP;
    }
    size_t n = 0;
    r = hiprtcGetCodeSize(prog, &n);
    if (r == HIPRTC_SUCCESS) { code.resize(n); r = hiprtcGetCode(prog, code.data()); }
    hiprtcDestroyProgram(&prog);
    if (r != HIPRTC_SUCCESS || code.empty()) { rl_set_error("%s: hiprtcGetCode: %s", who, hiprtcGetErrorString(r)); return RLREP_ERR_HIP; }
    return 0;
}

extern "C" {

int32_t rlrep_simx_state_bytes(void) { return (int32_t)sizeof(rlrep_simx_state); }

int64_t rlrep_sim_kind_source(const rlrep_sim_kind_desc* desc, char* text_out, int64_t cap) {
    if (!desc_check("sim_kind_source", desc)) return RLREP_ERR_ARG;
    const std::string t = assemble(desc);
    if (text_out && cap > 0) {
        const size_t n = std::min((size_t)cap - 1, t.size());
        memcpy(text_out, t.data(), n);
        text_out[n] = 0;
    }
    return (int64_t)t.size();
}

int32_t rlrep_sim_kind_code(const rlrep_sim_kind_desc* desc, const char* arch, void* code_out, int64_t cap, int64_t* size_out) {
    if (!desc_check("sim_kind_code", desc)) return RLREP_ERR_ARG;
    if (!arch || !arch[0] || !size_out) { rl_set_error("sim_kind_code: bad argument (null architecture or size)"); return RLREP_ERR_ARG; }
    std::vector<char> code;
    const int rc = compile_code("sim_kind_code", desc, arch, code);
    if (rc) return rc;
    *size_out = (int64_t)code.size();
    if (code_out && cap > 0) memcpy(code_out, code.data(), std::min((size_t)cap, code.size()));
    return 0;
}

int32_t rlrep_sim_kind_compile(const rlrep_sim_kind_desc* desc, rlrep_sim_kind** kind_out) {
    if (!desc_check("sim_kind_compile", desc)) return RLREP_ERR_ARG;
    if (!kind_out) { rl_set_error("sim_kind_compile: bad argument (null kind_out)"); return RLREP_ERR_ARG; }
    *kind_out = nullptr;
    int dev = 0;
    hipDeviceProp_t prop;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipGetDeviceProperties(&prop, dev);
    if (e != hipSuccess) { rl_set_error("sim_kind_compile: %s", hipGetErrorString(e)); return RLREP_ERR_HIP; }
    std::string arch(prop.gcnArchName);                 // "gfx950:sramecc+:xnack-": the processor alone selects the target
    arch = arch.substr(0, arch.find(':'));
    std::vector<char> code;
    const int rc = compile_code("sim_kind_compile", desc, arch.c_str(), code);
    if (rc) return rc;
    rlrep_sim_kind* k = new rlrep_sim_kind();
    e = hipModuleLoadData(&k->mod, code.data());
    if (e != hipSuccess) { rl_set_error("sim_kind_compile: hipModuleLoadData: %s", hipGetErrorString(e)); delete k; return RLREP_ERR_HIP; }
    static const char* const names[3] = {"simx_start_jit", "simx_step_jit", "simx_step_ctl_jit"};
    for (int i = 0; i < 3 && e == hipSuccess; ++i) {
        e = hipModuleGetFunction(&k->fn[i], k->mod, names[i]);
        if (e == hipSuccess) e = hipFuncGetAttribute(&k->info.regs[i], HIP_FUNC_ATTRIBUTE_NUM_REGS, k->fn[i]);
        if (e == hipSuccess) e = hipFuncGetAttribute(&k->info.scratch_bytes[i], HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, k->fn[i]);
        if (e == hipSuccess) e = hipFuncGetAttribute(&k->info.lds_bytes[i], HIP_FUNC_ATTRIBUTE_SHARED_SIZE_BYTES, k->fn[i]);
    }
    if (e != hipSuccess) { rl_set_error("sim_kind_compile: %s", hipGetErrorString(e)); (void)hipModuleUnload(k->mod); delete k; return RLREP_ERR_HIP; }
    k->info.S = desc->S; k->info.A = desc->A; k->info.NX = desc->NX; k->info.limit = desc->limit; k->info.terminates = desc->terminates ? 1 : 0;
    *kind_out = k;
    return 0;
}

void rlrep_sim_kind_destroy(rlrep_sim_kind* kind) {
    if (!kind) return;
    (void)hipModuleUnload(kind->mod);
    delete kind;
}

int32_t rlrep_sim_kind_info(const rlrep_sim_kind* kind, rlrep_sim_kind_info_t* info_out) {
    if (!kind || !info_out) { rl_set_error("sim_kind_info: bad argument (null kind or info)"); return RLREP_ERR_ARG; }
    *info_out = kind->info;
    return 0;
}

}  // extern "C"

// what the three launches refuse alike
static bool simx_check(const char* who, const rlrep_sim_kind* k, const rlrep_simx_state* s) {
    if (!k) { rl_set_error("%s: bad argument (null kind)", who); return false; }
    if (!s || !s->x || !s->ep_return || !s->last_return || !s->t || !s->episodes || !s->starts || !s->obs) {
        rl_set_error("%s: bad argument (null simulator state or array)", who); return false;
    }
    if (s->n < 1 || s->n > RLREP_SIM_MAX_ENVS) { rl_set_error("%s: n %d outside [1, %d]", who, s->n, RLREP_SIM_MAX_ENVS); return false; }
    return true;
}

static int simx_launch(const char* who, const rlrep_sim_kind* k, int which, int n, void** args, void* stream) {
    ++g_rl_launches;
    const hipError_t e = hipModuleLaunchKernel(k->fn[which], (unsigned)((n + 255) / 256), 1, 1, 256, 1, 1, 0, (hipStream_t)stream, args, nullptr);
    if (e != hipSuccess) { rl_set_error("%s: hip error %d", who, (int)e); return RLREP_ERR_HIP; }
    return 0;
}

extern "C" {

int32_t rlrep_simx_start(const rlrep_sim_kind* kind, const rlrep_simx_state* sim, void* stream) {
    if (!simx_check("simx_start", kind, sim)) return RLREP_ERR_ARG;
    SimxState s; memcpy(&s, sim, sizeof(s));
    void* args[] = {&s};
    return simx_launch("simx_start", kind, 0, s.n, args, stream);
}

int32_t rlrep_simx_step(const rlrep_sim_kind* kind, const rlrep_simx_state* sim, const float* act, int64_t ld_act, float* next_obs, float* reward,
                        float* done, void* stream) {
    if (!simx_check("simx_step", kind, sim)) return RLREP_ERR_ARG;
    if (!act || !next_obs || !reward || !done) { rl_set_error("simx_step: bad argument (null actions or output array)"); return RLREP_ERR_ARG; }
    if (ld_act < kind->info.A) { rl_set_error("simx_step: ld_act %lld below the kind's A %d", (long long)ld_act, kind->info.A); return RLREP_ERR_ARG; }
    SimxState s; memcpy(&s, sim, sizeof(s));
    long long ld = ld_act;
    void* args[] = {&s, &act, &ld, &next_obs, &reward, &done};
    return simx_launch("simx_step", kind, 1, s.n, args, stream);
}

int32_t rlrep_simx_step_append_ctl(const rlrep_sim_kind* kind, const rlrep_simx_state* sim, const float* act, int64_t ld_act, float* ring_dev,
                                   int64_t max_size, int32_t row_floats, int32_t* size_dev, int64_t* ctl_dev, void* stream) {
    if (!simx_check("simx_step_append_ctl", kind, sim)) return RLREP_ERR_ARG;
    if (!act || !ring_dev || !ctl_dev) { rl_set_error("simx_step_append_ctl: bad argument (null actions, ring or loop record)"); return RLREP_ERR_ARG; }
    if (max_size <= 0 || max_size > INT32_MAX || sim->n > max_size) {
        rl_set_error("simx_step_append_ctl: n %d outside [1, max_size %lld]", sim->n, (long long)max_size); return RLREP_ERR_ARG;
    }
    const int S = kind->info.S, A = kind->info.A;
    if (ld_act < A) { rl_set_error("simx_step_append_ctl: ld_act %lld below the kind's A %d", (long long)ld_act, A); return RLREP_ERR_ARG; }
    if (row_floats != 2 * S + A + 2) { rl_set_error("simx_step_append_ctl: row %d is not 2 S + A + 2 (S %d, A %d)", row_floats, S, A); return RLREP_ERR_ARG; }
    SimxState s; memcpy(&s, sim, sizeof(s));
    long long ld = ld_act, cap = max_size;
    void* args[] = {&s, &act, &ld, &ring_dev, &cap, &size_dev, &ctl_dev};
    return simx_launch("simx_step_append_ctl", kind, 2, s.n, args, stream);
}

}  // extern "C"
