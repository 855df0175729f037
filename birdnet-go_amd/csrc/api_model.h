// The model handle, as api_model.cpp (create / destroy / diagnostics) and api_predict.cpp (the run entries) share it.
#pragma once
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "api_common.h"
#include "engine.h"

namespace bnhip {

// One worker thread per engine of a multi-device handle: the thread owns its device's HIP context binding
// (hipSetDevice is thread-local), runs one job at a time, never lets an exception escape.
struct Worker {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::function<int(std::string&)> job;
    bool pending = false, stop = false;
    int rc = 0;
    std::string err;

    void start(int device);
    void submit(std::function<int(std::string&)> j);
    int wait(std::string* e);
    ~Worker();
};

}  // namespace bnhip

// A handle owns one engine per device of its "devices" list (one for the plain "device" form).  Clips of a call are
// sharded index-contiguously over the engines (independent clips, no exchange step).
struct bnhip_model {
    std::vector<std::unique_ptr<bnhip::Engine>> engs;
    std::vector<std::unique_ptr<bnhip::Worker>> workers;   // parallel to engs when engs.size() > 1
    std::string replication = "host-upload";           // how engines 1.. got their weights: "rccl-broadcast" | "peer-copy"
    bnhip::Engine& eng() { return *engs[0]; }
    const bnhip::Engine& eng() const { return *engs[0]; }
};

namespace bnhip {

// runs f(engine, first_clip, clip_count, err) -> rc for every shard of [0, n_clips); multi-device handles run the shards
// concurrently on their worker threads
template <class F>
int shard_run(bnhip_model* m, int n_clips, F f) {
    const int n = (int)m->engs.size();
    std::string err;
    if (n == 1) {
        int rc = f(*m->engs[0], 0, n_clips, err);
        return rc ? set_err(rc, err) : BNHIP_OK;
    }
    std::vector<int> used;
    for (int g = 0, off = 0; g < n; g++) {
        int cnt = n_clips / n + (g < n_clips % n ? 1 : 0);
        if (cnt > 0) {
            Engine* e = m->engs[g].get();
            const int o = off;
            m->workers[g]->submit([f, e, o, cnt](std::string& er) { return f(*e, o, cnt, er); });
            used.push_back(g);
        }
        off += cnt;
    }
    int rc = 0;
    for (int g : used) { int r = m->workers[g]->wait(&err); if (r && !rc) rc = r; }
    return rc ? set_err(rc, err) : BNHIP_OK;
}

}  // namespace bnhip
