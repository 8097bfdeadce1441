// hjbx_user.hip -- user-defined systems: the open half of the reference's plugin surface (dynamics/dynamics_basic.py:64-94: any subclass may
// define get_M / get_C / get_G / get_B, or get_control_affine_matrix itself).  hjbx_system_create_from_source compiles the subclass's
// device-code snippet with hiprtc into the library's own streaming kernels (hjbx_user_kernels.hpp + hjbx_stream_kernels.hpp, embedded
// below as text), keeps the code object in the handle, and the entry points of hjbx_kernels.hip launch it through the module API.
//
// A handle that asked for it (hjbx_system_enable_matrix_cores) also gets the two persistent matrix-core kernels of the value network
// (controller/vhjb.py:17-60, 162-193, 201-202: network, its input gradient, the closed loop): a second translation unit,
// hjbx_user_mlp_kernels.hpp, compiled at the first call for each (head, activation) and kept in the handle; hjbx_mlp.hip and
// hjbx_softpd.hip hand an enabled user handle over to hjbx_user_value_grad / hjbx_user_rollout below.  The parameter gradient
// (hjbx_value_loss_grad_f32 / hjbx_value_loss_adam_f32) is a third unit, hjbx_user_train_kernels.hpp: the cooperative kernel k_train_coop
// for the user's struct, one unit per activation (PD head only), compiled at its first use and refused as a whole when one of its four
// kernels needs scratch; hjbx_train_coop.hip builds the arguments and launches it through hjbx_user_train_launch below.  The Hessian of the
// value network (hjbx_value_hessian_f32 / hjbx_softpd_value_hessian_f32) is a fourth unit, hjbx_user_hessian_kernels.hpp: k_value_hessian
// for the user's struct, one kernel per (head, activation), compiled at its first use; hjbx_hessian.hip and hjbx_softpd_hessian.hip hand an
// enabled user handle over to hjbx_user_value_hessian below.
//
// User-defined CONTROL LAWS (controller/controller_basic.py:1-5, the other plugin surface) are compiled the same way, at the end of this file:
// hjbx_user_controller_create builds one more unit, hjbx_user_controller_kernels.hpp, for one (system, law) pair -- the system built-in or
// user-defined -- as a code object of its own, owned by the controller handle.
//
// hiprtc is opened with dlopen at first use: libhjbx.so has no link-time dependency on it, and a process that never creates a user system
// never loads it.  Compilation needs no GPU (the CPU test compiles a snippet); modules are loaded per device at the first launch.
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <dlfcn.h>
#include <elf.h>

#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "hjbx_internal.hpp"
#include "hjbx_host.hpp"
#include "hjbx_mlp_kernels.hpp"   // host side: the by-value argument structs of the two matrix-core kernels, exactly as the device unit sees them
#include "hjbx_mlp_host.hpp"

// ---- the header texts handed to hiprtc, embedded at build time (host pass only) ------------------------------------------------------
// (symbol, file under csrc, the name an #include of the device units finds it by): written once; the .incbin lines, the declarations and
// the two arrays handed to hiprtcCreateProgram (compile_unit) are generated from this list
#define HJBX_EMBEDDED_HEADERS(X)                                                    \
    X(hjbx_src_systems, "hjbx_systems.hpp", "hjbx_systems.hpp")                     \
    X(hjbx_src_stream, "hjbx_stream_kernels.hpp", "hjbx_stream_kernels.hpp")        \
    X(hjbx_src_user, "hjbx_user_kernels.hpp", "hjbx_user_kernels.hpp")              \
    X(hjbx_src_user_mlp, "hjbx_user_mlp_kernels.hpp", "hjbx_user_mlp_kernels.hpp")  \
    X(hjbx_src_mlp_core, "hjbx_mlp_core.hpp", "hjbx_mlp_core.hpp")                  \
    X(hjbx_src_mlp_kernels, "hjbx_mlp_kernels.hpp", "hjbx_mlp_kernels.hpp")         \
    X(hjbx_src_mlp_x3, "hjbx_mlp_x3.hpp", "hjbx_mlp_x3.hpp")                        \
    X(hjbx_src_mlp_h2, "hjbx_mlp_h2.hpp", "hjbx_mlp_h2.hpp")                        \
    X(hjbx_src_train_coop, "hjbx_train_coop_kernels.hpp", "hjbx_train_coop_kernels.hpp") \
    X(hjbx_src_user_train, "hjbx_user_train_kernels.hpp", "hjbx_user_train_kernels.hpp") \
    X(hjbx_src_hessian_kernels, "hjbx_hessian_kernels.hpp", "hjbx_hessian_kernels.hpp") \
    X(hjbx_src_user_hessian, "hjbx_user_hessian_kernels.hpp", "hjbx_user_hessian_kernels.hpp") \
    X(hjbx_src_user_controller, "hjbx_user_controller_kernels.hpp", "hjbx_user_controller_kernels.hpp") \
    X(hjbx_src_abi, "../../include/hjbx.h", "hjbx.h")
#if !defined(__HIP_DEVICE_COMPILE__)
#ifndef HJBX_CSRC_DIR
#error "compile hjbx_user.hip with -DHJBX_CSRC_DIR=\"<absolute path of csrc>\""
#endif
#define HJBX_EMBED(sym, file, name)                                                                                               \
    asm(".pushsection .rodata\n.global " #sym "\n.type " #sym ", @object\n" #sym ":\n.incbin \"" HJBX_CSRC_DIR "/" file "\"\n.byte 0\n" \
        ".popsection\n");
HJBX_EMBEDDED_HEADERS(HJBX_EMBED)
#undef HJBX_EMBED
#endif
#define HJBX_DECLARE(sym, file, name) extern "C" const char sym[];
HJBX_EMBEDDED_HEADERS(HJBX_DECLARE)
#undef HJBX_DECLARE

// what hiprtc's built-in runtime header does not bring: the system headers the library's own headers include, as far as they use them
static const char kStubRuntime[] = "// hip/hip_runtime.h: provided by hiprtc itself\n";
static const char kStubStdint[] =
    "#pragma once\n"
    "typedef signed char int8_t; typedef unsigned char uint8_t; typedef short int16_t; typedef unsigned short uint16_t;\n"
    "typedef int int32_t; typedef unsigned int uint32_t; typedef long int64_t; typedef unsigned long uint64_t; typedef unsigned long uintptr_t;\n";
static const char kStubStddef[] =
    "#pragma once\n"
    "typedef unsigned long size_t;\n"
    "#ifndef offsetof\n#define offsetof(t, m) __builtin_offsetof(t, m)\n#endif\n";
static const char kStubTypeTraits[] =
    "#pragma once\n"
    "namespace std {\n"
    "template <bool C, class A, class B> struct conditional { using type = A; };\n"
    "template <class A, class B> struct conditional<false, A, B> { using type = B; };\n"
    "template <bool C, class A, class B> using conditional_t = typename conditional<C, A, B>::type;\n"
    "template <class T, T v> struct integral_constant { static constexpr T value = v; };\n"
    "}\n";
// hjbx_internal.hpp of the device units: the ABI's enums and constants, none of the host-side declarations
static const char kStubInternal[] = "#pragma once\n#include \"hjbx.h\"\n";

// ---- hiprtc through dlopen -----------------------------------------------------------------------------------------------------
namespace {
struct Rtc {
    decltype(&hiprtcCreateProgram) create = nullptr;
    decltype(&hiprtcCompileProgram) compile = nullptr;
    decltype(&hiprtcGetProgramLogSize) log_size = nullptr;
    decltype(&hiprtcGetProgramLog) log = nullptr;
    decltype(&hiprtcGetCodeSize) code_size = nullptr;
    decltype(&hiprtcGetCode) code = nullptr;
    decltype(&hiprtcDestroyProgram) destroy = nullptr;
    decltype(&hiprtcAddNameExpression) add_name = nullptr;
    decltype(&hiprtcGetLoweredName) lowered = nullptr;
    bool ok = false;
};

const Rtc& rtc() {
    static Rtc r;
    static std::once_flag once;
    std::call_once(once, [] {
        void* h = nullptr;
        for (const char* name : {"libhiprtc.so.7", "libhiprtc.so", "/opt/rocm/lib/libhiprtc.so"}) {
            h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (h) break;
        }
        if (!h) return;
#define HJBX_SYM(field, sym) r.field = reinterpret_cast<decltype(r.field)>(dlsym(h, #sym))
        HJBX_SYM(create, hiprtcCreateProgram); HJBX_SYM(compile, hiprtcCompileProgram); HJBX_SYM(log_size, hiprtcGetProgramLogSize);
        HJBX_SYM(log, hiprtcGetProgramLog); HJBX_SYM(code_size, hiprtcGetCodeSize); HJBX_SYM(code, hiprtcGetCode);
        HJBX_SYM(destroy, hiprtcDestroyProgram); HJBX_SYM(add_name, hiprtcAddNameExpression); HJBX_SYM(lowered, hiprtcGetLoweredName);
#undef HJBX_SYM
        r.ok = r.create && r.compile && r.log_size && r.log && r.code_size && r.code && r.destroy && r.add_name && r.lowered;
    });
    return r;
}

thread_local std::string g_compile_log;

// one code object of a handle and what has been loaded from it, per device
struct UserUnit {
    std::vector<char> code;                          // the gfx950 code object
    hipModule_t mod[kMaxDevices] = {};
    std::map<std::string, hipFunction_t> fn[kMaxDevices];
    // a matrix-core unit only: 0 = not compiled yet, 1 = ready, -1 = the compile was refused (status, message and compiler log kept: a
    // second call reports them again instead of compiling for another 20 s)
    int state = 0, status = HJBX_OK;
    std::string error, log;
    std::string kernel[4];                           // symbols of: value gradient, Euler rollout, RK4 rollout (a train unit: index = 2 * residual mode + (PS == 4))
};

struct UserProgram {
    std::mutex mu;                                   // guards the module / function caches of every unit
    UserUnit stream;                                 // the streaming kernels (compiled at creation)
    // what the handle was created with: the matrix-core units are compiled from the same text and -D values, later
    std::string source;
    int user_kind = 0, n = 0, m = 0, np = 1;
    std::mutex mc_mu;                                // guards `matrix_cores` and the state of mc[][] (held across a lazy compile)
    bool matrix_cores = false;                       // hjbx_system_enable_matrix_cores
    UserUnit mc[2][3];                               // [head: 0 PD, 1 soft-PD][hjbx_activation]
    std::mutex train_mu;                             // guards the state of train[] (held across a lazy compile)
    UserUnit train[3];                               // [hjbx_activation]: the parameter-gradient unit (hjbx_user_train_kernels.hpp), PD head
    std::mutex hess_mu;                              // guards the state of hess[][] (held across a lazy compile)
    UserUnit hess[2][3];                             // [head][hjbx_activation]: the value-Hessian unit (hjbx_user_hessian_kernels.hpp); [1][relu] stays empty
};

// Compile `top` (one #include line) for the user's snippet with the library's own flags + `extra`; name expressions are resolved into
// out->kernel[].  `law` is the second in-memory header, "hjbx_user_law_snippet.hpp": the control law of hjbx_user_controller_kernels.hpp
// (empty for every other unit; `snippet` is empty for a law on a built-in system).
// Returns HJBX_OK with out->code filled; otherwise the hiprtc log is in g_compile_log and the error is set.
int compile_unit(const Rtc& R, const char* who, const char* top, const char* unit_name, const std::string& snippet, const std::string& law,
                 int user_kind, int n, int m, int np, const std::vector<std::string>& extra, const std::vector<const char*>& name_exprs,
                 UserUnit* out) {
#define HJBX_TEXT(sym, file, name) sym,
#define HJBX_NAME(sym, file, name) name,
    static const char kNone[] = "// (none)\n";   // (hiprtc refuses a header without text)
    const char* headers[] = {HJBX_EMBEDDED_HEADERS(HJBX_TEXT) kStubInternal, snippet.empty() ? kNone : snippet.c_str(), law.empty() ? kNone : law.c_str(), kStubRuntime, kStubStdint, kStubStddef, kStubStddef,
                             kStubTypeTraits};
    const char* names[] = {HJBX_EMBEDDED_HEADERS(HJBX_NAME) "hjbx_internal.hpp", "hjbx_user_snippet.hpp", "hjbx_user_law_snippet.hpp", "hip/hip_runtime.h", "stdint.h", "stddef.h",
                           "cstddef", "type_traits"};
#undef HJBX_TEXT
#undef HJBX_NAME
    static_assert(sizeof(headers) == sizeof(names), "one name per header");
    hiprtcProgram prog = nullptr;
    if (R.create(&prog, top, unit_name, (int)(sizeof(headers) / sizeof(headers[0])), headers, names) != HIPRTC_SUCCESS)
        return hjbx_set_error(HJBX_EHIP, "%s: hiprtcCreateProgram failed", who);
    for (const char* e : name_exprs)
        if (R.add_name(prog, e) != HIPRTC_SUCCESS) { R.destroy(&prog); return hjbx_set_error(HJBX_EHIP, "%s: hiprtcAddNameExpression(%s) failed", who, e); }
    // the flags of the library's own build: -ffp-contract=on keeps a user system's fused rollout bit-identical to its step kernels
    std::vector<std::string> o = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=on", "-DHJBX_USER_N=" + std::to_string(n),
                                  "-DHJBX_USER_M=" + std::to_string(m), "-DHJBX_USER_NP=" + std::to_string(np),
                                  "-DHJBX_USER_KIND=" + std::to_string(user_kind)};
    o.insert(o.end(), extra.begin(), extra.end());
    std::vector<const char*> opts;
    for (const std::string& f : o) opts.push_back(f.c_str());
    const hiprtcResult rc = R.compile(prog, (int)opts.size(), opts.data());
    size_t ls = 0;
    if (R.log_size(prog, &ls) == HIPRTC_SUCCESS && ls > 1) {
        g_compile_log.resize(ls);
        if (R.log(prog, &g_compile_log[0]) != HIPRTC_SUCCESS) g_compile_log.clear();
    }
    if (rc != HIPRTC_SUCCESS) {
        R.destroy(&prog);
        return hjbx_set_error(HJBX_EINVAL, "%s: the device source does not compile (hjbx_last_compile_log has the compiler's messages): %.300s", who,
                              g_compile_log.c_str());
    }
    size_t cs = 0;
    if (R.code_size(prog, &cs) != HIPRTC_SUCCESS || cs == 0) { R.destroy(&prog); return hjbx_set_error(HJBX_EHIP, "%s: no code object", who); }
    out->code.resize(cs);
    hiprtcResult rg = R.code(prog, out->code.data());
    for (size_t i = 0; rg == HIPRTC_SUCCESS && i < name_exprs.size() && i < 4; ++i) {
        const char* low = nullptr;
        rg = R.lowered(prog, name_exprs[i], &low);
        if (rg == HIPRTC_SUCCESS && low) out->kernel[i] = low;
    }
    R.destroy(&prog);
    if (rg != HIPRTC_SUCCESS) { out->code.clear(); return hjbx_set_error(HJBX_EHIP, "%s: hiprtcGetCode / hiprtcGetLoweredName failed", who); }
    return HJBX_OK;
}

// PRIVATE_SEGMENT_FIXED_SIZE (bytes 4..7 of the kernel descriptor, symbol `<kernel>.kd`) of a kernel in an AMDGPU code object: the bytes
// of scratch per work-item, i.e. whether the register allocator spilled VGPRs.  -1 when the symbol is not found.
long kernel_scratch_bytes(const std::vector<char>& code, const std::string& kernel) {
    Elf64_Ehdr eh;
    if (code.size() < sizeof eh) return -1;
    memcpy(&eh, code.data(), sizeof eh);
    if (memcmp(eh.e_ident, ELFMAG, SELFMAG) != 0 || eh.e_ident[EI_CLASS] != ELFCLASS64 || eh.e_shentsize != sizeof(Elf64_Shdr)) return -1;
    if (eh.e_shoff > code.size() || (size_t)eh.e_shnum * sizeof(Elf64_Shdr) > code.size() - eh.e_shoff) return -1;
    std::vector<Elf64_Shdr> sh(eh.e_shnum);
    if (eh.e_shnum) memcpy(sh.data(), code.data() + eh.e_shoff, sh.size() * sizeof(Elf64_Shdr));
    auto inside = [&](const Elf64_Shdr& s) { return s.sh_offset <= code.size() && s.sh_size <= code.size() - s.sh_offset; };
    const std::string want = kernel + ".kd";
    for (const Elf64_Shdr& st : sh) {
        if ((st.sh_type != SHT_SYMTAB && st.sh_type != SHT_DYNSYM) || st.sh_link >= sh.size() || !inside(st) || !inside(sh[st.sh_link])) continue;
        const Elf64_Shdr& str = sh[st.sh_link];
        for (size_t k = 0; k + sizeof(Elf64_Sym) <= st.sh_size; k += sizeof(Elf64_Sym)) {
            Elf64_Sym sym;
            memcpy(&sym, code.data() + st.sh_offset + k, sizeof sym);
            if (sym.st_name >= str.sh_size || sym.st_shndx >= sh.size()) continue;
            const char* nm = code.data() + str.sh_offset + sym.st_name;
            if (strnlen(nm, str.sh_size - sym.st_name) != want.size() || memcmp(nm, want.data(), want.size()) != 0) continue;
            const Elf64_Shdr& sec = sh[sym.st_shndx];
            if (!inside(sec) || sym.st_value < sec.sh_addr || sym.st_value - sec.sh_addr + 8 > sec.sh_size) return -1;
            uint32_t priv = 0;
            memcpy(&priv, code.data() + sec.sh_offset + (sym.st_value - sec.sh_addr) + 4, 4);
            return (long)priv;
        }
    }
    return -1;
}

// Launch `kernel` of `unit`: `grid` workgroups of `block` threads on `stream`; the module is loaded on the current device on first use
// (`mu` guards the unit's module / function caches).
int launch_unit(std::mutex& mu, UserUnit& unit, const char* kernel, unsigned grid, unsigned block, void** args, void* stream, const char* who) {
    const int dev = hjbx_current_device();
    if (dev < 0) return hjbx_set_error(HJBX_ENODEVICE, "%s: no HIP device", who);
    hipFunction_t f = nullptr;
    {
        std::lock_guard<std::mutex> lock(mu);
        if (!unit.mod[dev]) {
            const hipError_t e = hipModuleLoadData(&unit.mod[dev], unit.code.data());
            if (e != hipSuccess) { unit.mod[dev] = nullptr; return hjbx_set_error(HJBX_EHIP, "hipModuleLoadData: %s", hipGetErrorString(e)); }
        }
        auto it = unit.fn[dev].find(kernel);
        if (it == unit.fn[dev].end()) {
            const hipError_t e = hipModuleGetFunction(&f, unit.mod[dev], kernel);
            if (e != hipSuccess) return hjbx_set_error(HJBX_EHIP, "hipModuleGetFunction(%s): %s", kernel, hipGetErrorString(e));
            unit.fn[dev][kernel] = f;
        } else {
            f = it->second;
        }
    }
    const hipError_t e = hipModuleLaunchKernel(f, grid, 1, 1, block, 1, 1, 0, (hipStream_t)stream, args, nullptr);
    if (e != hipSuccess) return hjbx_set_error(HJBX_EHIP, "%s: %s", who, hipGetErrorString(e));
    return HJBX_OK;
}

void unload_unit(UserUnit& unit) {
    for (int d = 0; d < kMaxDevices; ++d)
        if (unit.mod[d]) (void)hipModuleUnload(unit.mod[d]);
}

// What a lazily compiled unit is made from, and how its refusal is worded
struct UnitSpec {
    const char *top, *name;                          // the one #include line, the unit's file name for hiprtc
    std::vector<std::string> flags;                  // -D values beyond those of the handle
    std::vector<const char*> kernels, labels;        // name expressions (resolved into UserUnit::kernel[]) and what the messages call them
    std::string variant;                             // "activation 1, PD head": follows n and m in the scratch refusal
    const char* budget;                              // what the kernels' code has to fit: ends the scratch refusal
};

// `unit` of handle `u`, compiled from make_spec() now if this is the first call that needs it (the caller holds the mutex of the unit's
// state); every later call costs the state test alone: the spec, with its strings, is built for the compile only.
// A kernel that needs scratch is a kernel that must not be launched: the whole unit is refused, its code object dropped, and the refusal
// remembered with its status, message and compiler log.
template <typename MakeSpec> int lazy_unit(UserProgram* u, UserUnit& unit, MakeSpec&& make_spec, const char* who, UserUnit** out) {
    if (unit.state == 0) {
        const UnitSpec spec = make_spec();
        g_compile_log.clear();
        const Rtc& R = rtc();   // (loaded: the handle was created through it)
        int rc = compile_unit(R, who, spec.top, spec.name, u->source, std::string(), u->user_kind, u->n, u->m, u->np, spec.flags, spec.kernels, &unit);
        for (size_t k = 0; rc == HJBX_OK && k < spec.kernels.size(); ++k) {
            const long scratch = kernel_scratch_bytes(unit.code, unit.kernel[k]);
            if (scratch < 0) rc = hjbx_set_error(HJBX_EHIP, "%s: kernel %s is missing from the compiled code object", who, unit.kernel[k].c_str());
            else if (scratch > 0)
                rc = hjbx_set_error(HJBX_EUNSUPPORTED, "%s: the %s kernel of this user system (n=%d m=%d, %s) needs %ld bytes of scratch: its code does not fit %s",
                                    who, spec.labels[k], u->n, u->m, spec.variant.c_str(), scratch, spec.budget);
        }
        unit.state = rc == HJBX_OK ? 1 : -1;
        unit.status = rc;
        unit.log = g_compile_log;
        if (rc != HJBX_OK) {
            char msg[512];
            hjbx_last_error(msg, sizeof msg);
            unit.error = msg;
            unit.code.clear();
        }
    }
    if (unit.state < 0) {
        g_compile_log = unit.log;
        return hjbx_set_error(unit.status, "%s", unit.error.c_str());
    }
    *out = &unit;
    return HJBX_OK;
}

// The matrix-core unit of an enabled handle for (head, activation), compiled now if this is the first call that needs it.
int matrix_core_unit(const hjbx_system* s, int soft, int act, const char* who, UserUnit** out) {
    UserProgram* u = s->kind == HJBX_SYS_USER ? static_cast<UserProgram*>(s->user) : nullptr;
    if (!u) return hjbx_set_error(HJBX_EINVAL, "%s: not a user-defined system", who);
    if (soft < 0 || soft > 1 || act < 0 || act > 2) return hjbx_set_error(HJBX_EINVAL, "%s: unknown head %d / activation %d", who, soft, act);
    std::lock_guard<std::mutex> lock(u->mc_mu);
    if (!u->matrix_cores)
        return hjbx_set_error(HJBX_EUNSUPPORTED, "%s: this user-defined system has not asked for the matrix-core kernels (hjbx_system_enable_matrix_cores)", who);
    // Two waves per SIMD leave 256 registers per lane and the kernels keep a whole layer in them: a spill to scratch is a kernel that
    // must not be launched (a spill store inside an EXEC-predicated region once produced wrong trajectories here)
    return lazy_unit(u, u->mc[soft][act], [&] { return
                     UnitSpec{"#include \"hjbx_user_mlp_kernels.hpp\"\n", "hjbx_user_matrix_cores.hip",
                              {"-DHJBX_USER_MLP_ACT=" + std::to_string(act), "-DHJBX_USER_MLP_SOFT=" + std::to_string(soft)},
                              {"HJBX_UM_VALUE_GRAD", "HJBX_UM_ROLLOUT_EULER", "HJBX_UM_ROLLOUT_RK4"}, {"value-gradient", "Euler rollout", "RK4 rollout"},
                              "activation " + std::to_string(act) + (soft ? ", soft-PD head" : ", PD head"), "the 256 registers of the matrix-core kernels"}; },
                     who, out);
}

// The train unit of an enabled handle for `act`, compiled now if this is the first call that needs it.  One wave per SIMD and 512 registers:
// when ANY of the four kernels needs scratch the whole unit is refused (a controller trains fused or it does not), the code object is
// dropped and the refusal remembered; the handle keeps its streaming and rollout units.
int train_unit(const hjbx_system* s, int act, const char* who, UserUnit** out) {
    UserProgram* u = s->kind == HJBX_SYS_USER ? static_cast<UserProgram*>(s->user) : nullptr;
    if (!u) return hjbx_set_error(HJBX_EINVAL, "%s: not a user-defined system", who);
    if (act < 0 || act > 2) return hjbx_set_error(HJBX_EINVAL, "%s: unknown activation %d", who, act);
    if (s->n % 2)
        return hjbx_set_error(HJBX_EUNSUPPORTED, "%s: the fused parameter gradient needs an even state dimension (k-steps of 2), got n=%d", who, s->n);
    if (!hjbx_user_matrix_cores(s))
        return hjbx_set_error(HJBX_EUNSUPPORTED, "%s: this user-defined system has not asked for the matrix-core kernels (hjbx_system_enable_matrix_cores)", who);
    if (act == HJBX_ACT_SIN && s->n > 4)
        return hjbx_set_error(HJBX_EUNSUPPORTED, "%s: the sin network's fused parameter gradient exists for n <= 4 (n = %d)", who, s->n);
    std::lock_guard<std::mutex> lock(u->train_mu);
    // (the library's common flags only: with -fno-slp-vectorize, which hjbx_train_coop.hip's own build adds, hiprtc's compiler needs
    //  16-72 bytes of scratch for the tanh / sin kernels of the test systems)
    return lazy_unit(u, u->train[act], [&] { return
                     UnitSpec{"#include \"hjbx_user_train_kernels.hpp\"\n", "hjbx_user_train.hip", {"-DHJBX_USER_MLP_ACT=" + std::to_string(act)},
                              {"HJBX_UT_M0_PS1", "HJBX_UT_M0_PS4", "HJBX_UT_M1_PS1", "HJBX_UT_M1_PS4"},
                              {"k_train_coop<mode 0, PS 1>", "k_train_coop<mode 0, PS 4>", "k_train_coop<mode 1, PS 1>", "k_train_coop<mode 1, PS 4>"},
                              "activation " + std::to_string(act),
                              "the 512 registers of the cooperative parameter-gradient kernel; the fused parameter gradient is refused for this system"}; },
                     who, out);
}

// The value-Hessian unit of an enabled handle for (head, activation), compiled now if this is the first call that needs it: one kernel, one
// wave per SIMD and 512 registers; when it needs scratch the unit is refused, the code object dropped and the refusal remembered -- the handle
// keeps its streaming, matrix-core and train units.  No soft-PD ReLU unit exists: that Hessian is identically zero.
int hessian_unit(const hjbx_system* s, int soft, int act, const char* who, UserUnit** out) {
    UserProgram* u = s->kind == HJBX_SYS_USER ? static_cast<UserProgram*>(s->user) : nullptr;
    if (!u) return hjbx_set_error(HJBX_EINVAL, "%s: not a user-defined system", who);
    if (soft < 0 || soft > 1 || act < 0 || act > 2) return hjbx_set_error(HJBX_EINVAL, "%s: unknown head %d / activation %d", who, soft, act);
    if (!hjbx_user_matrix_cores(s))
        return hjbx_set_error(HJBX_EUNSUPPORTED, "%s: this user-defined system has not asked for the matrix-core kernels (hjbx_system_enable_matrix_cores)", who);
    if (soft && act == HJBX_ACT_RELU)
        return hjbx_set_error(HJBX_EUNSUPPORTED, "%s: the Hessian of a soft-PD ReLU network is identically zero (H is filled with zeros): there is no kernel and no code object", who);
    std::lock_guard<std::mutex> lock(u->hess_mu);
    return lazy_unit(u, u->hess[soft][act], [&] { return
                     UnitSpec{"#include \"hjbx_user_hessian_kernels.hpp\"\n", "hjbx_user_hessian.hip",
                              {"-DHJBX_USER_MLP_ACT=" + std::to_string(act), "-DHJBX_USER_MLP_SOFT=" + std::to_string(soft)},
                              {"HJBX_UH_VALUE_HESSIAN"}, {"value-Hessian"},
                              "activation " + std::to_string(act) + (soft ? ", soft-PD head" : ", PD head"), "the 512 registers of the Hessian kernel"}; },
                     who, out);
}
}  // namespace

extern "C" size_t hjbx_last_compile_log(char* buf, size_t buflen) {
    const size_t len = g_compile_log.size();
    if (buf && buflen) {
        const size_t n = len < buflen - 1 ? len : buflen - 1;
        memcpy(buf, g_compile_log.data(), n);
        buf[n] = '\0';
    }
    return len;
}

void hjbx_user_release(void* up) {
    UserProgram* u = static_cast<UserProgram*>(up);
    if (!u) return;
    unload_unit(u->stream);
    for (auto& head : u->mc)
        for (UserUnit& unit : head) unload_unit(unit);
    for (UserUnit& unit : u->train) unload_unit(unit);
    for (auto& head : u->hess)
        for (UserUnit& unit : head) unload_unit(unit);
    delete u;
}

extern "C" int hjbx_system_create_from_source(int user_kind, const char* device_source, int n, int m, double dt, const double* umin,
                                              const double* umax, const double* params, int n_params, hjbx_system** out) {
    if (!out) return hjbx_set_error(HJBX_EINVAL, "out is NULL");
    *out = nullptr;
    g_compile_log.clear();
    if (user_kind != HJBX_USER_AFFINE && user_kind != HJBX_USER_MANIPULATOR) return hjbx_set_error(HJBX_EINVAL, "unknown user system kind %d", user_kind);
    if (!device_source || !umin || !umax) return hjbx_set_error(HJBX_EINVAL, "device_source / umin / umax must be non-NULL");
    if (n < 1 || n > HJBX_MAX_N || m < 1 || m > HJBX_MAX_M) return hjbx_set_error(HJBX_EINVAL, "user system needs 1<=n<=%d, 1<=m<=%d", HJBX_MAX_N, HJBX_MAX_M);
    if (user_kind == HJBX_USER_MANIPULATOR && n % 2) return hjbx_set_error(HJBX_EINVAL, "a manipulator state is (q, dq): n must be even, got %d", n);
    if (n_params < 0 || n_params > HJBX_USER_MAX_PARAMS || (n_params > 0 && !params))
        return hjbx_set_error(HJBX_EINVAL, "user system takes 0..%d parameters", HJBX_USER_MAX_PARAMS);
    if (!(dt > 0) || !(dt < 1e300)) return hjbx_set_error(HJBX_EINVAL, "dt must be positive and finite");
    for (int j = 0; j < m; ++j)
        if (!(umin[j] <= umax[j])) return hjbx_set_error(HJBX_EINVAL, "umin[%d] > umax[%d]", j, j);
    const Rtc& R = rtc();
    if (!R.ok) {
        const char* why = dlerror();       // (one call: dlerror clears the message it returns)
        return hjbx_set_error(HJBX_EUNSUPPORTED, "hjbx_system_create_from_source: libhiprtc.so could not be loaded (%s)", why ? why : "symbols missing");
    }
    UserProgram* u = new (std::nothrow) UserProgram();
    if (!u) return hjbx_set_error(HJBX_EINVAL, "out of host memory");
    u->source = device_source; u->user_kind = user_kind; u->n = n; u->m = m; u->np = n_params > 0 ? n_params : 1;
    if (int rc = compile_unit(R, "hjbx_system_create_from_source", "#include \"hjbx_user_kernels.hpp\"\n", "hjbx_user_system.hip", u->source, std::string(),
                              user_kind, n, m, u->np, {}, {}, &u->stream)) {
        delete u;
        return rc;
    }
    hjbx_system* s = new_system(HJBX_SYS_USER, n, m, dt, umin, umax, params, n_params, u);
    if (!s) { delete u; return hjbx_set_error(HJBX_EINVAL, "out of host memory"); }
    *out = s;
    return HJBX_OK;
}

extern "C" int hjbx_system_enable_matrix_cores(hjbx_system* sys) {
    if (!sys) return hjbx_set_error(HJBX_EINVAL, "hjbx_system_enable_matrix_cores: system handle is NULL");
    UserProgram* u = sys->kind == HJBX_SYS_USER ? static_cast<UserProgram*>(sys->user) : nullptr;
    if (!u) return hjbx_set_error(HJBX_EINVAL, "hjbx_system_enable_matrix_cores: a built-in system has its matrix-core kernels already (user-defined systems only)");
    if (sys->n % 2)
        return hjbx_set_error(HJBX_EUNSUPPORTED, "hjbx_system_enable_matrix_cores: the matrix-core kernels need an even state dimension (k-steps of 2), got n=%d", sys->n);
    if (sys->n > HJBX_MAX_N || sys->m > HJBX_MAX_M)
        return hjbx_set_error(HJBX_EUNSUPPORTED, "hjbx_system_enable_matrix_cores: the matrix-core kernels take n<=%d, m<=%d", HJBX_MAX_N, HJBX_MAX_M);
    std::lock_guard<std::mutex> lock(u->mc_mu);
    u->matrix_cores = true;
    return HJBX_OK;
}

bool hjbx_user_matrix_cores(const hjbx_system* s) {
    UserProgram* u = s && s->kind == HJBX_SYS_USER ? static_cast<UserProgram*>(s->user) : nullptr;
    if (!u) return false;
    std::lock_guard<std::mutex> lock(u->mc_mu);
    return u->matrix_cores;
}

extern "C" int hjbx_system_matrix_cores(const hjbx_system* sys) { return hjbx_user_matrix_cores(sys) ? 1 : 0; }

extern "C" size_t hjbx_system_code_object(const hjbx_system* sys, int which, void* buf, size_t len) {
    UserProgram* u = sys && sys->kind == HJBX_SYS_USER ? static_cast<UserProgram*>(sys->user) : nullptr;
    if (!u) { hjbx_set_error(HJBX_EINVAL, "hjbx_system_code_object: not a user-defined system"); return 0; }
    const UserUnit* unit = &u->stream;
    if (which != HJBX_CODE_STREAMING) {
        if (which < 1 || which > 15) { hjbx_set_error(HJBX_EINVAL, "hjbx_system_code_object: unknown code object %d", which); return 0; }
        UserUnit* mc = nullptr;
        if (which >= 10) {
            if (hessian_unit(sys, (which - 10) / 3, (which - 10) % 3, "hjbx_system_code_object", &mc) != HJBX_OK) return 0;
        } else if (which >= 7) {
            if (train_unit(sys, which - 7, "hjbx_system_code_object", &mc) != HJBX_OK) return 0;
        } else if (matrix_core_unit(sys, (which - 1) / 3, (which - 1) % 3, "hjbx_system_code_object", &mc) != HJBX_OK) {
            return 0;
        }
        unit = mc;
    }
    if (buf && len) memcpy(buf, unit->code.data(), len < unit->code.size() ? len : unit->code.size());
    return unit->code.size();
}

// Launch `kernel` (an extern "C" name of hjbx_user_kernels.hpp) of this handle's streaming code object: `grid` workgroups of 256 threads on
// `stream`, args = pointers to the kernel's arguments in order (the first one a UserBlob).
int hjbx_user_launch(const hjbx_system* s, const char* kernel, unsigned grid, void** args, void* stream) {
    UserProgram* u = static_cast<UserProgram*>(s->user);
    if (!u) return hjbx_set_error(HJBX_EINVAL, "system handle has no user program");
    return launch_unit(u->mu, u->stream, kernel, grid, 256, args, stream, kernel);
}

// ---- the matrix-core kernels of an enabled handle --------------------------------------------------------------------------------
namespace {
constexpr unsigned kMcBlock = 8 * 64;   // WAVES * 64 of hjbx_user_mlp_kernels.hpp
}  // namespace

int hjbx_user_value_grad(const hjbx_system* s, const hjbx_net& net, const float* x, float* V, float* g, int64_t B, void* stream, const char* who) {
    UserUnit* unit = nullptr;
    if (int rc = matrix_core_unit(s, net.soft, net.activation, who, &unit)) return rc;
    return with_mc_dims(s, who, "matrix-core kernel", [&](auto Nc, auto) -> int {
        constexpr int N = decltype(Nc)::value;
        auto blob = user_blob<float>(s);
        MlpP<N> p = make_mlp_params<N>(net);
        int64_t ngroups = 0, grid = 0;
        if (int rc = mlp_persistent_grid(B, 32, &ngroups, &grid, who)) return rc;
        MlpHeadSoft soft = make_head<MlpHeadSoft>(net);
        MlpHeadPd pd{};
        void* a[] = {&blob, &p, (void*)&net.W1, (void*)&net.W2, (void*)&net.W3, (void*)&x, (void*)&V, (void*)&g, (void*)&B, &ngroups,
                     net.soft ? (void*)&soft : (void*)&pd};
        return launch_unit(static_cast<UserProgram*>(s->user)->mu, *unit, unit->kernel[0].c_str(), (unsigned)grid, kMcBlock, a, stream, who);
    });
}

int hjbx_user_rollout(const hjbx_system* s, const hjbx_task* task, const hjbx_net& net, const hjbx_rollout_args& r, const char* who) {
    if (r.integrator != HJBX_EULER && r.integrator != HJBX_RK4) return hjbx_set_error(HJBX_EUNSUPPORTED, "%s: a user system steps with HJBX_EULER or HJBX_RK4", who);
    UserUnit* unit = nullptr;
    if (int rc = matrix_core_unit(s, net.soft, net.activation, who, &unit)) return rc;
    return with_mc_dims(s, who, "matrix-core kernel", [&](auto Nc, auto Mc) -> int {
        constexpr int N = decltype(Nc)::value, M = decltype(Mc)::value;
        auto blob = user_blob<float>(s);
        MlpP<N> p = make_mlp_params<N>(net);
        auto tk = make_task<float, N, M>(task);
        auto lim = make_limits<float, M>(s);
        RolloutOut<N, M> o{r.traj, r.u_log, r.cost, r.done, r.resid, r.done_step, r.x_out};
        int64_t ngroups = 0, grid = 0;
        int sched = 0;
        if (int rc = mlp_rollout_grid(r.B, &ngroups, &grid, &sched, who)) return rc;
        unsigned* ws = (unsigned*)r.workspace;
        MlpHeadSoft soft = make_head<MlpHeadSoft>(net);
        MlpHeadPd pd{};
        void* a[] = {&blob, &p, &tk, &lim, (void*)&net.W1, (void*)&net.W2, (void*)&net.W3, (void*)&r.t_first, (void*)&r.n_steps, (void*)&r.T_max, (void*)&r.x,
                     (void*)&r.env_order, &o, (void*)&r.B, &ngroups, &ws, &sched, net.soft ? (void*)&soft : (void*)&pd};
        return launch_unit(static_cast<UserProgram*>(s->user)->mu, *unit, unit->kernel[r.integrator == HJBX_RK4 ? 2 : 1].c_str(), (unsigned)grid, kMcBlock, a,
                           r.stream, who);
    });
}

// ---- the value-network Hessian of an enabled handle (called by hjbx_hessian.hip / hjbx_softpd_hessian.hip after check_value_hessian) ---------
// launch_value_hessian of hjbx_mlp_host.hpp for the handle's own unit: 32 / n samples per tile group, kHessWaves waves per workgroup
int hjbx_user_value_hessian(const hjbx_system* s, const hjbx_net& net, const float* x, float* H, float* dy, int64_t B, void* stream, const char* who) {
    UserUnit* unit = nullptr;
    if (int rc = hessian_unit(s, net.soft, net.activation, who, &unit)) return rc;
    return with_mc_dims(s, who, "Hessian kernel", [&](auto Nc, auto) -> int {
        constexpr int N = decltype(Nc)::value;
        auto blob = user_blob<float>(s);
        MlpP<N> p = make_mlp_params<N>(net);
        int64_t ngroups = 0, grid = 0;
        if (int rc = mlp_persistent_grid(B, 32 / N, &ngroups, &grid, who)) return rc;
        MlpHeadSoft soft = make_head<MlpHeadSoft>(net);
        MlpHeadPd pd{};
        void* a[] = {&blob, &p, (void*)&net.W1, (void*)&net.W2, (void*)&net.W3, (void*)&x, (void*)&H, (void*)&dy, (void*)&B, &ngroups,
                     net.soft ? (void*)&soft : (void*)&pd};
        return launch_unit(static_cast<UserProgram*>(s->user)->mu, *unit, unit->kernel[0].c_str(), (unsigned)grid, kHessWaves * 64, a, stream, who);
    });
}

// ---- the parameter gradient of an enabled handle (called by hjbx_train_coop.hip) ----------------------------------------------------
int hjbx_user_train_unit(const hjbx_system* s, int activation, const char* who) {
    UserUnit* unit = nullptr;
    return train_unit(s, activation, who, &unit);
}

int hjbx_user_train_launch(const hjbx_system* s, int activation, int mode, int psplit, unsigned grid, void** args, void* stream, const char* who) {
    if (mode < 0 || mode > 1 || (psplit != 1 && psplit != 4)) return hjbx_set_error(HJBX_EINVAL, "%s: residual mode %d / psplit %d", who, mode, psplit);
    UserUnit* unit = nullptr;
    if (int rc = train_unit(s, activation, who, &unit)) return rc;
    return launch_unit(static_cast<UserProgram*>(s->user)->mu, *unit, unit->kernel[2 * mode + (psplit == 4 ? 1 : 0)].c_str(), grid, 256, args, stream, who);
}

// ---- user-defined control laws (hjbx_user_controller_*, include/hjbx.h) -----------------------------------------------------------
// The reference's second plugin surface (controller/controller_basic.py:1-5) in the closed loop of controller/vhjb.py:171-193: one code
// object per (system, law) pair, hjbx_user_controller_kernels.hpp compiled around the law's snippet -- and around the system's own snippet
// when the system is user-defined.  The controller COPIES what it needs from the system handle (kind, dimensions, parameters, limits, dt,
// the system's snippet and its -D values): it shares nothing with the handle and outlives it.
struct hjbx_user_controller {
    hjbx_system sys;                    // a copy of the handle's plain data; `user` is NULL here
    std::string sys_source;             // HJBX_SYS_USER: the system's snippet
    int user_kind = 0, np = 1;
    std::mutex mu;                      // guards the unit's module / function caches and q
    UserUnit unit;
    double q[HJBX_LAW_MAX_PARAMS];
    int n_q = 0, n_w = 0, has_reached = 0;
};

namespace {
#define HJBX_UC_REQUIRE(cond, ...)                                    \
    do {                                                              \
        if (!(cond)) return hjbx_set_error(HJBX_EINVAL, __VA_ARGS__); \
    } while (0)

const char* const kLawKernels[2][3] = {{"hjbx_uc_control_f32", "hjbx_uc_rollout_i0_f32", "hjbx_uc_rollout_i1_f32"},
                                       {"hjbx_uc_control_f64", "hjbx_uc_rollout_i0_f64", "hjbx_uc_rollout_i1_f64"}};

// the law's parameters as the kernels take them: UserLaw<T, S> is `struct { T q[NQ]; }`
template <typename T> struct LawBlob { T q[HJBX_LAW_MAX_PARAMS]; };
template <typename T> LawBlob<T> law_blob(hjbx_user_controller* c) {
    LawBlob<T> b;
    std::lock_guard<std::mutex> lock(c->mu);
    for (int i = 0; i < HJBX_LAW_MAX_PARAMS; ++i) b.q[i] = i < c->n_q ? (T)c->q[i] : T(0);
    return b;
}
template <typename S> const void* system_arg(const S& s) {
    if constexpr (is_user<S>::value) return &s.blob;
    else return &s;
}

template <typename T>
int user_controller_eval(hjbx_user_controller* c, const T* x, const T* w, double t, T* u, int64_t B, void* stream) {
    const char* who = "hjbx_user_controller_eval";
    HJBX_UC_REQUIRE(c != nullptr, "%s: controller handle is NULL", who);
    HJBX_UC_REQUIRE(B >= 0, "%s: negative batch size %lld", who, (long long)B);
    if (B == 0) return HJBX_OK;
    const hjbx_system* s = &c->sys;
    HJBX_UC_REQUIRE(x != nullptr && aligned_rows(x, (size_t)s->n * sizeof(T)), "%s: x must be a non-NULL device pointer aligned to its row vector width", who);
    HJBX_UC_REQUIRE(u != nullptr && aligned_rows(u, (size_t)s->m * sizeof(T)), "%s: u must be a non-NULL device pointer aligned to its row vector width", who);
    HJBX_UC_REQUIRE(c->n_w == 0 || (w != nullptr && aligned_rows(w, (size_t)c->n_w * sizeof(T))),
                    "%s: this law reads %d per-environment values: w must be a non-NULL (B, %d) device pointer aligned to its row vector width", who, c->n_w, c->n_w);
    return with_any_system<T>(s, [&](auto S) -> int {
        using SS = decltype(S);
        auto law = law_blob<T>(c);
        auto lim = make_limits<T, SS::M>(s);
        T tt = (T)t;
        void* a[] = {const_cast<void*>(system_arg(S)), &law, &lim, &tt, (void*)&x, (void*)&w, (void*)&u, (void*)&B};
        return launch_unit(c->mu, c->unit, kLawKernels[sizeof(T) == 8][0], (unsigned)((B + 255) / 256), 256, a, stream, who);
    });
}

// every argument check of hjbx_rollout_feedback_* (rollout_feedback_impl, hjbx_kernels.hip), before any launch
template <typename T>
int user_controller_rollout(hjbx_user_controller* c, const hjbx_task* task, int integ, uint32_t flags, double t0, int T_steps, const T* x0,
                            const T* w, T* traj, T* u_log, T* cost, int32_t* done_step, T* total_cost, T* x_final, int64_t B, void* stream) {
    const char* who = "hjbx_user_controller_rollout";
    HJBX_UC_REQUIRE(c != nullptr, "%s: controller handle is NULL", who);
    HJBX_UC_REQUIRE(B >= 0, "%s: negative batch size %lld", who, (long long)B);
    if (B == 0) return HJBX_OK;
    const hjbx_system* s = &c->sys;
    if (integ == HJBX_ZOH) return hjbx_set_error(HJBX_EUNSUPPORTED, "%s: HJBX_ZOH stepping is not built for user-defined control laws (HJBX_EULER or HJBX_RK4)", who);
    HJBX_UC_REQUIRE(integ == HJBX_EULER || integ == HJBX_RK4, "%s: unknown integrator %d", who, integ);
    HJBX_UC_REQUIRE(T_steps >= 0, "%s: negative horizon", who);
    HJBX_UC_REQUIRE((flags & ~(HJBX_ROLLOUT_TERMINATE | HJBX_ROLLOUT_STOP_AT_TARGET)) == 0, "%s: unknown rollout flags 0x%x", who, flags);
    HJBX_UC_REQUIRE(task || !(flags & HJBX_ROLLOUT_TERMINATE), "%s: HJBX_ROLLOUT_TERMINATE needs a task", who);
    if (task) { if (int rc = check_task(task)) return rc; }
    HJBX_UC_REQUIRE(task || (!cost && !total_cost), "%s: cost outputs need a task", who);
    HJBX_UC_REQUIRE(c->has_reached || !(flags & HJBX_ROLLOUT_STOP_AT_TARGET), "%s: HJBX_ROLLOUT_STOP_AT_TARGET needs a law that defines `reached`", who);
    HJBX_UC_REQUIRE(x0 != nullptr && aligned_rows(x0, (size_t)s->n * sizeof(T)), "%s: x0 must be a non-NULL device pointer aligned to its row vector width", who);
    HJBX_UC_REQUIRE(c->n_w == 0 || (w != nullptr && aligned_rows(w, (size_t)c->n_w * sizeof(T))),
                    "%s: this law reads %d per-environment values: w must be a non-NULL (B, %d) device pointer aligned to its row vector width", who, c->n_w, c->n_w);
    HJBX_UC_REQUIRE(!traj || aligned_rows(traj, (size_t)s->n * sizeof(T)), "%s: traj must be aligned to its row vector width", who);
    HJBX_UC_REQUIRE(!u_log || aligned_rows(u_log, (size_t)s->m * sizeof(T)), "%s: u_log must be aligned to its row vector width", who);
    HJBX_UC_REQUIRE(!x_final || aligned_rows(x_final, (size_t)s->n * sizeof(T)), "%s: x_final must be aligned to its row vector width", who);
    return with_any_system<T>(s, [&](auto S) -> int {
        using SS = decltype(S);
        auto law = law_blob<T>(c);
        auto tk = make_task<T, SS::N, SS::M>(task);
        auto lim = make_limits<T, SS::M>(s);
        int has_task = task != nullptr;
        T tt = (T)t0;
        void* a[] = {const_cast<void*>(system_arg(S)), &law, &tk, &lim, &flags, &has_task, &T_steps, &tt, (void*)&x0, (void*)&w, (void*)&traj, (void*)&u_log,
                     (void*)&cost, (void*)&done_step, (void*)&total_cost, (void*)&x_final, (void*)&B};
        return launch_unit(c->mu, c->unit, kLawKernels[sizeof(T) == 8][integ == HJBX_RK4 ? 2 : 1], (unsigned)((B + 255) / 256), 256, a, stream, who);
    });
}
}  // namespace

extern "C" int hjbx_user_controller_create(const hjbx_system* sys, const char* law_source, const double* q, int n_q, int n_w, int has_reached,
                                           hjbx_user_controller** out) {
    const char* who = "hjbx_user_controller_create";
    if (!out) return hjbx_set_error(HJBX_EINVAL, "%s: out is NULL", who);
    *out = nullptr;
    g_compile_log.clear();
    HJBX_UC_REQUIRE(sys != nullptr && law_source != nullptr, "%s: sys / law_source must be non-NULL", who);
    HJBX_UC_REQUIRE(n_q >= 0 && n_q <= HJBX_LAW_MAX_PARAMS && (n_q == 0 || q), "%s: a control law takes 0..%d parameters, got %d", who, HJBX_LAW_MAX_PARAMS, n_q);
    HJBX_UC_REQUIRE(n_w >= 0 && n_w <= HJBX_LAW_MAX_ENV_PARAMS, "%s: a control law takes 0..%d per-environment values, got %d", who, HJBX_LAW_MAX_ENV_PARAMS, n_w);
    HJBX_UC_REQUIRE(sys->kind >= HJBX_SYS_LINEAR && sys->kind <= HJBX_SYS_USER, "%s: unknown system kind %d", who, sys->kind);
    const UserProgram* up = sys->kind == HJBX_SYS_USER ? static_cast<const UserProgram*>(sys->user) : nullptr;
    if (sys->kind == HJBX_SYS_USER) {
        HJBX_UC_REQUIRE(up != nullptr, "%s: system handle has no user program", who);
    } else if (!with_system<float>(sys, [](auto) {})) {
        return hjbx_set_error(HJBX_EUNSUPPORTED, "%s: no kernel for system kind %d with n=%d m=%d", who, sys->kind, sys->n, sys->m);
    }
    const Rtc& R = rtc();
    if (!R.ok) {
        const char* why = dlerror();
        return hjbx_set_error(HJBX_EUNSUPPORTED, "%s: libhiprtc.so could not be loaded (%s)", who, why ? why : "symbols missing");
    }
    hjbx_user_controller* c = new (std::nothrow) hjbx_user_controller();
    if (!c) return hjbx_set_error(HJBX_EINVAL, "out of host memory");
    c->sys = *sys;
    c->sys.user = nullptr;
    if (up) { c->sys_source = up->source; c->user_kind = up->user_kind; c->np = up->np; }
    for (int i = 0; i < HJBX_LAW_MAX_PARAMS; ++i) c->q[i] = i < n_q ? q[i] : 0.0;
    c->n_q = n_q; c->n_w = n_w; c->has_reached = has_reached ? 1 : 0;
    const std::vector<std::string> flags = {"-DHJBX_LAW_SYSTEM=" + std::to_string(sys->kind), "-DHJBX_LAW_NQ=" + std::to_string(n_q > 0 ? n_q : 1),
                                            "-DHJBX_LAW_NW=" + std::to_string(n_w), "-DHJBX_LAW_HAS_REACHED=" + std::to_string(c->has_reached)};
    int rc = compile_unit(R, who, "#include \"hjbx_user_controller_kernels.hpp\"\n", "hjbx_user_controller.hip", c->sys_source, law_source, c->user_kind,
                          sys->n, sys->m, c->np, flags, {}, &c->unit);
    // scratch is reported, not refused: a streaming kernel that spills is slow, not wrong
    for (int p = 0; rc == HJBX_OK && p < 2; ++p)
        for (int k = 0; rc == HJBX_OK && k < 3; ++k) {
            const long scratch = kernel_scratch_bytes(c->unit.code, kLawKernels[p][k]);
            if (scratch < 0) rc = hjbx_set_error(HJBX_EHIP, "%s: kernel %s is missing from the compiled code object", who, kLawKernels[p][k]);
            else if (scratch > 0) g_compile_log += "note: " + std::string(kLawKernels[p][k]) + " needs " + std::to_string(scratch) + " bytes of scratch per lane\n";
        }
    if (rc != HJBX_OK) { delete c; return rc; }
    *out = c;
    return HJBX_OK;
}

extern "C" void hjbx_user_controller_destroy(hjbx_user_controller* c) {
    if (!c) return;
    unload_unit(c->unit);
    delete c;
}

extern "C" int hjbx_user_controller_set_params(hjbx_user_controller* c, const double* q, int n_q) {
    HJBX_UC_REQUIRE(c != nullptr, "hjbx_user_controller_set_params: controller handle is NULL");
    HJBX_UC_REQUIRE(n_q == c->n_q && (n_q == 0 || q), "hjbx_user_controller_set_params: this law was compiled for %d parameters, got %d", c->n_q, n_q);
    std::lock_guard<std::mutex> lock(c->mu);
    for (int i = 0; i < n_q; ++i) c->q[i] = q[i];
    return HJBX_OK;
}

extern "C" size_t hjbx_user_controller_code_object(const hjbx_user_controller* c, void* buf, size_t len) {
    if (!c) { hjbx_set_error(HJBX_EINVAL, "hjbx_user_controller_code_object: controller handle is NULL"); return 0; }
    if (buf && len) memcpy(buf, c->unit.code.data(), len < c->unit.code.size() ? len : c->unit.code.size());
    return c->unit.code.size();
}

extern "C" int hjbx_user_controller_eval_f32(hjbx_user_controller* c, const float* x, const float* w, double t, float* u, int64_t B, void* stream) {
    return user_controller_eval<float>(c, x, w, t, u, B, stream);
}
extern "C" int hjbx_user_controller_eval_f64(hjbx_user_controller* c, const double* x, const double* w, double t, double* u, int64_t B, void* stream) {
    return user_controller_eval<double>(c, x, w, t, u, B, stream);
}
extern "C" int hjbx_user_controller_rollout_f32(hjbx_user_controller* c, const hjbx_task* task, int integrator, uint32_t flags, double t0, int T_steps,
                                                const float* x0, const float* w, float* traj, float* u_log, float* cost, int32_t* done_step,
                                                float* total_cost, float* x_final, int64_t B, void* stream) {
    return user_controller_rollout<float>(c, task, integrator, flags, t0, T_steps, x0, w, traj, u_log, cost, done_step, total_cost, x_final, B, stream);
}
extern "C" int hjbx_user_controller_rollout_f64(hjbx_user_controller* c, const hjbx_task* task, int integrator, uint32_t flags, double t0, int T_steps,
                                                const double* x0, const double* w, double* traj, double* u_log, double* cost, int32_t* done_step,
                                                double* total_cost, double* x_final, int64_t B, void* stream) {
    return user_controller_rollout<double>(c, task, integrator, flags, t0, T_steps, x0, w, traj, u_log, cost, done_step, total_cost, x_final, B, stream);
}
