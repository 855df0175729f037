// C ABI of the model handle: options, create / destroy (with the weight replication and worker threads of a multi-device
// handle), info, stream binding and the profiling / describe diagnostics.  The run entries are in api_predict.cpp.
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "api_model.h"
#include "model_onnx.h"
#include "tflite_model.h"

using namespace bnhip;

namespace bnhip {

void Worker::start(int device) {
    th = std::thread([this, device] {
        hipSetDevice(device);
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            cv.wait(lk, [this] { return pending || stop; });
            if (stop) return;
            std::function<int(std::string&)> j = std::move(job);
            lk.unlock();
            int r; std::string e;
            try { r = j(e); }
            catch (...) { r = exception_error(e); }
            lk.lock();
            rc = r; err.swap(e); pending = false;
            cv.notify_all();
        }
    });
}
void Worker::submit(std::function<int(std::string&)> j) {
    std::lock_guard<std::mutex> lk(mu);
    job = std::move(j); pending = true; rc = 0; err.clear();
    cv.notify_all();
}
int Worker::wait(std::string* e) {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [this] { return !pending; });
    if (rc && e && e->empty()) *e = err;
    return rc;
}
Worker::~Worker() {
    if (th.joinable()) {
        { std::lock_guard<std::mutex> lk(mu); stop = true; cv.notify_all(); }
        th.join();
    }
}

}  // namespace bnhip

namespace {

// ---------------------------------------------------------------------------------------------- options
// tiny extractors for flat {"key": value} options.  -> the text of key's value, nullptr when the key is absent
const char* json_find(const char* js, const char* key) {
    if (!js) return nullptr;
    std::string pat = std::string("\"") + key + "\"";
    const char* p = strstr(js, pat.c_str());
    if (!p) return nullptr;
    p += pat.size();
    while (*p == ' ' || *p == ':' || *p == '\t') p++;
    return p;
}
// {"key": <int>}; absent -> def
long json_int(const char* js, const char* key, long def) {
    const char* p = json_find(js, key);
    if (!p) return def;
    char* end = nullptr;
    long v = strtol(p, &end, 10);
    return end == p ? def : v;
}
// {"key": [i, j, ...]} -> values; absent or malformed -> empty
std::vector<int> json_int_array(const char* js, const char* key) {
    std::vector<int> v;
    const char* p = json_find(js, key);
    if (!p || *p != '[') return v;
    p++;
    while (*p && *p != ']') {
        char* end = nullptr;
        long x = strtol(p, &end, 10);
        if (end == p) { v.clear(); return v; }
        v.push_back((int)x);
        p = end;
        while (*p == ' ' || *p == ',' || *p == '\t') p++;
    }
    return v;
}
// {"key": "text"} -> text; absent -> def
std::string json_str(const char* js, const char* key, const char* def) {
    const char* p = json_find(js, key);
    if (!p || *p != '"') return def;
    const char* q = strchr(p + 1, '"');
    return q ? std::string(p + 1, q) : std::string(def);
}

// What a handle's options JSON says, read once per create.  Where a BNHIP_* environment variable is named it is the
// experiment switch behind the option: the option wins when given, the variable when not, the default otherwise.
struct ModelOptions {
    // "plan_only": parse + plan on the CPU, no device touched (diagnostics / CPU-side tests); such a
    // model answers info/describe and rejects predict calls.
    bool plan_only;
    std::vector<int> devices;
    int max_batch;
    bool no_reuse, autotune, use_graphs;
    int n_lanes, depth, host_depth, frontend_fft, bf16x3, logits_output, embedding_output;
    std::string tune_dir, precision, replicate;

    explicit ModelOptions(const char* js) {
        auto num = [js](const char* key, const char* env, long def) {
            const char* e = env ? getenv(env) : nullptr;
            return json_int(js, key, e ? atoi(e) : def);
        };
        auto text = [js](const char* key, const char* env, const char* def) {
            const char* e = env ? getenv(env) : nullptr;
            return json_str(js, key, e ? e : def);
        };
        plan_only = num("plan_only", nullptr, 0) != 0;
        devices = json_int_array(js, "devices");
        if (devices.empty()) devices.push_back((int)num("device", nullptr, 0));
        max_batch = (int)num("max_batch", nullptr, 256);
        no_reuse = num("debug_no_reuse", nullptr, 0) != 0;
        autotune = num("autotune", nullptr, 1) != 0;
        tune_dir = text("tune_dir", "BNHIP_TUNE_DIR", "");
        n_lanes = (int)num("lanes", "BNHIP_LANES", 2);
        depth = (int)num("depth", "BNHIP_DEPTH", 1);
        host_depth = (int)num("host_depth", "BNHIP_HOST_DEPTH", 2);
        frontend_fft = (int)num("frontend_fft", "BNHIP_FE_FFT", -1);
        use_graphs = num("graphs", "BNHIP_GRAPHS", 0) != 0;
        // default 1: per layer where the create-time autotuner measures the split-bf16 kernel faster (fp32-equivalent
        // products; tests/test_bf16x3.py holds the error comparison against the float64 arbiter that decided the default)
        bf16x3 = (int)num("bf16x3", "BNHIP_BF16X3", 1);
        logits_output = (int)num("logits_output", nullptr, -1);
        embedding_output = (int)num("embedding_output", nullptr, -2);      // -1: no embedding; -2: the family rule
        // "precision": "f32" (default) | "bf16": MFMA operands rounded to bf16, fp32 accumulate and storage (BASELINE
        // configs[4] asks for this on Perch; never the default: v2.4 in reduced precision is known to fail, model_openvino.go:99-103)
        precision = text("precision", "BNHIP_PRECISION", "f32");
        replicate = text("replicate", nullptr, "auto");
    }
    bool precision_known() const { return precision == "f32" || precision == "bf16"; }
    void apply(Engine& e) const {
        e.no_reuse = no_reuse; e.autotune = autotune; e.tune_dir = tune_dir;
        e.n_lanes = n_lanes; e.depth = depth; e.host_depth = host_depth;
        e.frontend_fft = frontend_fft; e.use_graphs = use_graphs;
        e.logits_output = logits_output; e.embedding_output = embedding_output;
        e.precision = precision == "bf16" ? 1 : 0;
        e.bf16x3 = e.precision && !bf16x3 ? 1 : bf16x3;      // the bf16 kernels read the split weight images' first plane
    }
};

// BNHIP_DUMP_IR diagnostics: the operator list the planner will see
void dump_ir(const TflModel& tm) {
    auto tensor = [&tm](const char* kind, int t) {
        fprintf(stderr, " %s%d[", kind, t);
        for (size_t k = 0; k < tm.tensors[t].shape.size(); k++) fprintf(stderr, "%s%d", k ? "," : "", tm.tensors[t].shape[k]);
        fprintf(stderr, "]");
    };
    for (size_t oi = 0; oi < tm.ops.size(); oi++) {
        const TflOp& o = tm.ops[oi];
        fprintf(stderr, "[bnhip] ir %3zu %-18s", oi, op_name(o.code));
        for (int t : o.inputs) {
            if (t < 0) fprintf(stderr, " -");
            else tensor(tm.tensors[t].data ? "c" : "t", t);
        }
        fprintf(stderr, " ->");
        for (int t : o.outputs) tensor("t", t);
        fprintf(stderr, "\n");
    }
}

// ---------------------------------------------------------------------------------------------- RCCL (optional, dlopen'd)
// Weights of a multi-device handle are uploaded to the first device only and replicated device-to-device: RCCL
// ncclBroadcast over xGMI when librccl is loadable and the devices are distinct, hipMemcpyPeer otherwise.  The library is
// resolved at run time so libbnhip.so itself links against nothing but the HIP runtime.
struct Rccl {
    void* h = nullptr;
    int (*CommInitAll)(void**, int, const int*) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Broadcast)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    bool load() {
        if (h) return true;
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"}) {
            h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (h) break;
        }
        if (!h) return false;
        *(void**)&CommInitAll = dlsym(h, "ncclCommInitAll");
        *(void**)&CommDestroy = dlsym(h, "ncclCommDestroy");
        *(void**)&GroupStart = dlsym(h, "ncclGroupStart");
        *(void**)&GroupEnd = dlsym(h, "ncclGroupEnd");
        *(void**)&Broadcast = dlsym(h, "ncclBroadcast");
        *(void**)&GetErrorString = dlsym(h, "ncclGetErrorString");
        if (!CommInitAll || !CommDestroy || !GroupStart || !GroupEnd || !Broadcast) { dlclose(h); h = nullptr; return false; }
        return true;
    }
};
Rccl g_rccl;
std::mutex g_rccl_mu;

// returns "" on success (and sets *how), else an error text
std::string replicate_weights(bnhip_model* m, const std::string& mode, std::string* how) {
    const int n = (int)m->engs.size();
    Engine& root = *m->engs[0];
    const size_t bytes = root.weights_bytes();
    bool distinct = true;
    for (int i = 0; i < n; i++)
        for (int j = i + 1; j < n; j++) if (m->engs[i]->device == m->engs[j]->device) distinct = false;
    bool want_rccl = mode == "rccl" || (mode == "auto" && distinct && n > 1);
    if (want_rccl && !distinct) return "replicate=rccl needs distinct devices";
    if (want_rccl) {
        std::lock_guard<std::mutex> lk(g_rccl_mu);
        if (!g_rccl.load()) {
            if (mode == "rccl") return "replicate=rccl requested but librccl could not be loaded";
            want_rccl = false;
        } else {
            std::vector<int> devs(n);
            for (int i = 0; i < n; i++) devs[i] = m->engs[i]->device;
            std::vector<void*> comms(n, nullptr);
            int rc = g_rccl.CommInitAll(comms.data(), n, devs.data());
            if (rc == 0) {
                rc = g_rccl.GroupStart();
                for (int i = 0; i < n && rc == 0; i++) {
                    hipSetDevice(devs[i]);
                    // count in 4-byte words (ncclFloat32 == 7); root sends in place
                    rc = g_rccl.Broadcast(root.weights_ptr(), m->engs[i]->weights_ptr(), (bytes + 3) / 4, 7, 0, comms[i],
                                          m->engs[i]->stream);
                }
                int rc2 = g_rccl.GroupEnd();
                if (rc == 0) rc = rc2;
                for (int i = 0; i < n; i++) { hipSetDevice(devs[i]); hipStreamSynchronize(m->engs[i]->stream); }
                for (int i = 0; i < n; i++) if (comms[i]) g_rccl.CommDestroy(comms[i]);
            }
            hipSetDevice(devs[0]);
            if (rc == 0) { *how = "rccl-broadcast"; return ""; }
            if (mode == "rccl")
                return std::string("RCCL broadcast failed: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "?");
            want_rccl = false;          // auto: fall through to peer copies
        }
    }
    for (int i = 1; i < n; i++) {
        Engine& e = *m->engs[i];
        hipError_t he;
        if (e.device == root.device) he = hipMemcpy(e.weights_ptr(), root.weights_ptr(), bytes, hipMemcpyDeviceToDevice);
        else he = hipMemcpyPeer(e.weights_ptr(), e.device, root.weights_ptr(), root.device, bytes);
        if (he != hipSuccess) return std::string("weight peer copy failed: ") + hipGetErrorString(he);
    }
    hipSetDevice(root.device);
    *how = n > 1 ? "peer-copy" : "host-upload";
    return "";
}

}  // namespace

extern "C" {

int bnhip_model_create(const void* blob, size_t n_bytes, const char* opts_json, bnhip_model** out) {
    if (!out) return set_err(BNHIP_E_INVALID, "out is NULL");
    *out = nullptr;
    bnhip_model* m = nullptr;
    BN_GUARD_BEGIN
    if (!blob || n_bytes == 0) return set_err(BNHIP_E_INVALID, "empty model blob");
    const ModelOptions opt(opts_json);
    const std::vector<int>& devices = opt.devices;
    if (devices.size() > 64) return set_err(BNHIP_E_INVALID, "too many devices");
    if (opt.max_batch < 1 || opt.max_batch > 4096) return set_err(BNHIP_E_INVALID, "max_batch must be in [1, 4096]");
    if (!opt.plan_only) {
        int rc = bnhip_init(nullptr);
        if (rc != BNHIP_OK) return rc;
        for (int device : devices) {
            if (device < 0 || device >= device_count()) return set_err(BNHIP_E_INVALID, "device ordinal out of range");
            if (!is_gfx950(device)) return set_err(BNHIP_E_NO_DEVICE, "selected device is not gfx950");
        }
    }

    // container: TFLite flatbuffer ("TFL3" at byte 4) or ONNX protobuf (internal/inference/onnx/classifier.go:268-430)
    TflModel tm;
    std::string err;
    const bool is_tfl = n_bytes >= 8 && memcmp((const char*)blob + 4, "TFL3", 4) == 0;
    if (is_tfl) {
        if (!parse_tflite(blob, n_bytes, &tm, &err)) return set_err(BNHIP_E_MODEL, err);
    } else {
        int ocode = BNHIP_E_MODEL;
        if (!parse_onnx(blob, n_bytes, &tm, &err, &ocode)) return set_err(ocode, err);
    }
    if (getenv("BNHIP_DUMP_IR")) dump_ir(tm);
    if (!validate_graph(tm, &err)) return set_err(BNHIP_E_MODEL, err);
    if (!opt.precision_known()) return set_err(BNHIP_E_INVALID, "precision must be \"f32\" or \"bf16\"");

    m = new bnhip_model();
    const int n_eng = (int)devices.size();
    for (int i = 0; i < n_eng; i++) {
        std::unique_ptr<Engine> e(new Engine());
        opt.apply(*e);
        e->defer_weights = i > 0 && !opt.plan_only;
        int code = BNHIP_E_UNSUPPORTED;
        TflModel copy = tm;                               // tensors point into the caller's blob / tm-owned storage: cheap
        if (!e->build(std::move(copy), devices[i], opt.max_batch, opt.plan_only, &err, &code)) {
            delete m;
            return set_err(code == BNHIP_OK ? BNHIP_E_UNSUPPORTED : code, err);
        }
        m->engs.push_back(std::move(e));
    }
    if (n_eng > 1 && !opt.plan_only) {
        std::string how;
        std::string rerr = replicate_weights(m, opt.replicate, &how);
        if (!rerr.empty()) { delete m; return set_err(BNHIP_E_RUNTIME, rerr); }
        m->replication = how;
        for (int i = 0; i < n_eng; i++) {
            m->workers.emplace_back(new Worker());
            m->workers.back()->start(devices[i]);
        }
        // create-time autotune of the deferred engines, concurrently on their own devices
        for (int i = 1; i < n_eng; i++) {
            Engine* e = m->engs[i].get();
            m->workers[i]->submit([e](std::string&) { e->finish_deferred(); return 0; });
        }
        for (int i = 1; i < n_eng; i++) m->workers[i]->wait(nullptr);
        hipSetDevice(devices[0]);
    } else if (n_eng == 1 && !opt.plan_only && opt.replicate == "rccl") {
        // single device, RCCL explicitly requested: run the broadcast code path with one rank (in place) so that the
        // library load and call sequence are exercised on a one-GPU box
        std::string how;
        std::string rerr = replicate_weights(m, "rccl", &how);
        if (!rerr.empty()) { delete m; return set_err(BNHIP_E_RUNTIME, rerr); }
        m->replication = how;
    }
    *out = m;
    return BNHIP_OK;
    BN_GUARD_END(delete m)
}

int bnhip_model_info(const bnhip_model* m, int* n_samples, int* n_classes, int* emb_dim) {
    if (!m) return set_err(BNHIP_E_INVALID, "model is NULL");
    if (n_samples) *n_samples = m->eng().n_samples;
    if (n_classes) *n_classes = m->eng().n_classes;
    if (emb_dim) *emb_dim = m->eng().emb_dim;
    return BNHIP_OK;
}

int bnhip_model_devices(const bnhip_model* m, int* devices, int cap) {
    if (!m) return set_err(BNHIP_E_INVALID, "model is NULL");
    const int n = (int)m->engs.size();
    for (int i = 0; i < n && i < cap && devices; i++) devices[i] = m->engs[i]->device;
    return n;
}

void bnhip_model_destroy(bnhip_model* m) {
    if (!m) return;
    try {
        m->workers.clear();                             // joins the worker threads first
        for (auto& e : m->engs) {
            if (e && e->device >= 0) hipSetDevice(e->device);
            e.reset();
        }
        delete m;
    } catch (...) {}
}

int bnhip_set_stream(bnhip_model* m, void* hip_stream) {
    if (!m || m->eng().device < 0) return set_err(BNHIP_E_INVALID, "model is NULL or plan-only");
    if (m->engs.size() > 1) return set_err(BNHIP_E_INVALID, "bnhip_set_stream: multi-device handles own their streams");
    BN_GUARD_BEGIN
    Engine& e = m->eng();
    hipSetDevice(e.device);
    e.drop_graphs();                                    // captured on the old stream
    e.sync_contexts();
    if (e.stream) hipStreamSynchronize(e.stream);       // (the engine keeps its own streams: contexts and lanes run on them)
    e.stream = reinterpret_cast<hipStream_t>(hip_stream);
    e.own_stream = false;
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

int bnhip_synchronize(bnhip_model* m) {
    if (!m || m->eng().device < 0) return set_err(BNHIP_E_INVALID, "model is NULL or plan-only");
    BN_GUARD_BEGIN
    for (auto& ep : m->engs) {
        Engine& e = *ep;
        hipSetDevice(e.device);
        e.sync_contexts();
        hipError_t he = hipStreamSynchronize(e.stream);
        if (he != hipSuccess) return set_err(BNHIP_E_RUNTIME, std::string("hipStreamSynchronize: ") + hipGetErrorString(he));
    }
    hipSetDevice(m->eng().device);
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

// ------------------------------------------------------------------------------------------------ diagnostics
int bnhip_profile_enable(bnhip_model* m, int on) {
    if (!m) return set_err(BNHIP_E_INVALID, "model is NULL");
    m->eng().profiling = on != 0;
    return BNHIP_OK;
}

int bnhip_profile_filter(bnhip_model* m, const char* kernel_class) {
    if (!m) return set_err(BNHIP_E_INVALID, "model is NULL");
    BN_GUARD_BEGIN
    m->eng().profile_filter = kernel_class ? kernel_class : "";
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

int bnhip_profile_read(bnhip_model* m, char* buf, size_t cap) {
    if (!m || m->eng().device < 0) return set_err(BNHIP_E_INVALID, "model is NULL or plan-only");
    BN_GUARD_BEGIN
    hipSetDevice(m->eng().device);
    return copy_out(m->eng().profile_read(), buf, cap);
    BN_GUARD_END((void)0)
}

int bnhip_profile_steps(bnhip_model* m, int on) {
    if (!m) return set_err(BNHIP_E_INVALID, "model is NULL");
    m->eng().step_timing = on != 0;
    return BNHIP_OK;
}

int bnhip_profile_steps_read(bnhip_model* m, double* start_ms, double* end_ms, int cap) {
    if (!m || m->eng().device < 0) return set_err(BNHIP_E_INVALID, "model is NULL or plan-only");
    if (cap < 0) return set_err(BNHIP_E_INVALID, "negative capacity");
    BN_GUARD_BEGIN
    hipSetDevice(m->eng().device);
    return m->eng().steps_read(start_ms, end_ms, cap);
    BN_GUARD_END((void)0)
}

int bnhip_model_describe(const bnhip_model* m, char* buf, size_t cap) {
    if (!m) return set_err(BNHIP_E_INVALID, "model is NULL");
    BN_GUARD_BEGIN
    std::string d = m->eng().describe();
    // splice the handle-level facts in front of the engine's description
    std::string devs = "[";
    for (size_t i = 0; i < m->engs.size(); i++) devs += (i ? "," : "") + std::to_string(m->engs[i]->device);
    devs += "]";
    // (what every engine of the handle runs: one tuning adopted by all of them, or their own - "tune_sources"; "plans_identical":
    // every engine picked the same tile / kernel form for every step, so a clip's bits do not depend on the shard it lands on)
    std::string srcs = "[";
    bool same = true;
    for (size_t i = 0; i < m->engs.size(); i++) {
        srcs += std::string(i ? "," : "") + "\"" + m->engs[i]->tune_source + "\"";
        same = same && m->engs[i]->tuning_text() == m->engs[0]->tuning_text();
    }
    srcs += "]";
    std::string head = "{\"devices\":" + devs + ",\"weight_replication\":\"" + m->replication + "\",\"tune_sources\":" + srcs +
                       ",\"plans_identical\":" + (same ? "true" : "false") + ",";
    if (!d.empty() && d[0] == '{') d = head + d.substr(1);
    return copy_out(d, buf, cap);
    BN_GUARD_END((void)0)
}

}  // extern "C"
