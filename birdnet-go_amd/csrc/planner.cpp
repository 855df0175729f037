// Plan time: the TFLite op graph -> Engine::steps / vals / specs, the activation arena layouts and the host image of the
// weight arena.  Pure CPU work (plan_only engines stop here); the device half of Engine::build - allocation, weight upload,
// pointer patching - is Engine::bind_device in engine.cpp; the bf16 storage decision and the create-time tuning that follow it are tune.cpp.
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

#include "../../include/bnhip.h"

namespace bnhip {

namespace {

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct Planner {
    const TflModel& m;
    std::vector<int> producer;                 // tensor -> op index (-1: const / input)
    std::vector<std::vector<int>> consumers;   // tensor -> op indices
    std::vector<int> uses;                     // consumer count + graph outputs
    std::vector<char> absorbed;                // op consumed by a fusion
    std::string err;

    explicit Planner(const TflModel& mm) : m(mm) {
        int nt = (int)m.tensors.size();
        producer.assign(nt, -1);
        consumers.assign(nt, {});
        uses.assign(nt, 0);
        absorbed.assign(m.ops.size(), 0);
        for (int i = 0; i < (int)m.ops.size(); i++) {
            if (m.ops[i].code == OP_NOP) { absorbed[i] = 1; continue; }      // removed by a graph pass
            for (int o : m.ops[i].outputs) producer[o] = i;
            for (int t : m.ops[i].inputs)
                if (t >= 0) { consumers[t].push_back(i); uses[t]++; }
        }
        for (int t : m.outputs) uses[t]++;
    }
    bool is_const(int t) const { return t >= 0 && m.tensors[t].data != nullptr; }
    const TflTensor& T(int t) const { return m.tensors[t]; }
    bool fail(const std::string& s) { if (err.empty()) err = s; return false; }

    static bool shape_op(int code) { return code == OP_RESHAPE || code == OP_EXPAND_DIMS || code == OP_SQUEEZE; }
    // tf.signal.frame slices the signal to a whole number of sub-frames first; when nothing is cut the
    // STRIDED_SLICE is an identity and is treated like a reshape
    bool identity_op(int oi) const {
        const TflOp& o = m.ops[oi];
        if (shape_op(o.code)) return true;
        return o.code == OP_STRIDED_SLICE && !o.inputs.empty() && !o.outputs.empty() &&
               m.tensors[o.inputs[0]].numel() == m.tensors[o.outputs[0]].numel();
    }

    int skip_up(int t) {          // walk producers through pure shape ops
        while (t >= 0 && producer[t] >= 0 && identity_op(producer[t])) {
            absorbed[producer[t]] = 1;
            t = m.ops[producer[t]].inputs[0];
        }
        return t;
    }
    int skip_down(int t) {        // walk single consumers through pure shape ops
        while (consumers[t].size() == 1 && identity_op(consumers[t][0])) {
            absorbed[consumers[t][0]] = 1;
            t = m.ops[consumers[t][0]].outputs[0];
        }
        return t;
    }
    int only_consumer(int t) const { return consumers[t].size() == 1 ? consumers[t][0] : -1; }
    int take(int oi) { absorbed[oi] = 1; return skip_down(m.ops[oi].outputs[0]); }   // absorb op oi, walk on from its output
    // scalar float const?
    bool const_scalar(int t, float* v) const {
        if (!is_const(t) || T(t).type != TT_FLOAT32 || T(t).numel() != 1) return false;
        *v = T(t).f32()[0];
        return true;
    }
    // binary op with one const-scalar operand: returns the other operand
    int bin_const(const TflOp& o, float* c, bool* const_is_rhs = nullptr) const {
        if (o.inputs.size() != 2) return -1;
        if (const_scalar(o.inputs[1], c)) { if (const_is_rhs) *const_is_rhs = true; return o.inputs[0]; }
        if (const_scalar(o.inputs[0], c)) { if (const_is_rhs) *const_is_rhs = false; return o.inputs[1]; }
        return -1;
    }
};

struct FrontendMatch {
    int L = 0, Lfft = 0, hop = 0, F = 0, n_mels = 0;
    std::vector<float> window;
    int mel_tensor = -1;     // const [n_mels, nbins]
    float p1 = 1.f, p2 = 1.f, eps = 0.f, norm_sub = 0.f, norm_mul = 1.f;
    bool reverse = false;
    bool magnitude = false;  // COMPLEX_ABS instead of the real part
    bool normalize = true;   // per-clip min/max normalisation in front of the framing (false: raw samples)
    int pad_left = 0, pad_right = 0;   // zero samples the graph PADs around the clip before framing
    bool log_compress = false;         // scale * log(max(x, floor)) instead of the two POWs
    float log_floor = 0.f, log_scale = 1.f;
    bool time_major = false; // image is [1, F, n_mels, 1] (no TRANSPOSE) instead of [1, n_mels, F, 1]
    int out_tensor = -1;     // [1, n_mels, F, 1] or [1, F, n_mels, 1]
};

// Recognise one MelSpec branch around RFFT2D op `ri` (see header comment in synth_model.py for the graph).
bool match_frontend(Planner& P, int ri, FrontendMatch* fm) {
    const TflModel& m = P.m;
    const TflOp& R = m.ops[ri];
    if (R.inputs.size() != 2 || !P.is_const(R.inputs[1]) || P.T(R.inputs[1]).numel() != 2)
        return P.fail("RFFT2D: fft_length must be a constant [2]");
    const int32_t* fl = P.T(R.inputs[1]).i32();
    if (fl[0] != 1) return P.fail("RFFT2D: only 1-D transforms (fft_length[0]==1) are supported");
    fm->Lfft = fl[1];
    P.absorbed[ri] = 1;

    // ---- upstream: window MUL <- framing GATHER <- normalisation chain <- graph input
    int t = P.skip_up(R.inputs[0]);
    int pi = P.producer[t];
    // frames shorter than the transform: tf.signal.stft zero-pads them at the end (PAD on the last axis only)
    if (pi >= 0 && m.ops[pi].code == OP_PAD) {
        const TflOp& pd = m.ops[pi];
        const TflTensor& pv = P.T(pd.inputs[1]);
        const int rank = (int)P.T(pd.inputs[0]).shape.size();
        if (!pv.data || (int)pv.numel() != 2 * rank) return P.fail("front-end: frame PAD needs constant paddings");
        for (int d = 0; d < 2 * rank - 1; d++)
            if (pv.i32()[d] != 0) return P.fail("front-end: frames may only be zero-padded at the end of the last axis");
        P.absorbed[pi] = 1;
        t = P.skip_up(pd.inputs[0]);
        pi = P.producer[t];
    }
    int frames_t = t;
    if (pi >= 0 && m.ops[pi].code == OP_MUL) {
        const TflOp& mu = m.ops[pi];
        int wc = P.is_const(mu.inputs[1]) ? 1 : (P.is_const(mu.inputs[0]) ? 0 : -1);
        if (wc < 0) return P.fail("front-end: window MUL without a constant operand");
        const TflTensor& wt = P.T(mu.inputs[wc]);
        if (wt.type != TT_FLOAT32) return P.fail("front-end: window must be float32");
        fm->window.assign(wt.f32(), wt.f32() + wt.numel());
        frames_t = mu.inputs[1 - wc];
        P.absorbed[pi] = 1;
    }
    t = P.skip_up(frames_t);
    pi = P.producer[t];
    if (pi < 0 || m.ops[pi].code != OP_GATHER) return P.fail("front-end: framing pattern (GATHER) not found");
    {
        const TflOp& ga = m.ops[pi];
        if (ga.axis != 1 || ga.batch_dims != 0 || !P.is_const(ga.inputs[1]) || P.T(ga.inputs[1]).shape.size() != 2)
            return P.fail("front-end: unsupported GATHER framing");
        const TflTensor& sel = P.T(ga.inputs[1]);
        const TflTensor& par = P.T(ga.inputs[0]);
        if (par.shape.size() != 3) return P.fail("front-end: GATHER params must be [1, n_sub, sub]");
        int sub = par.shape[2], F = sel.shape[0], Q = sel.shape[1];
        const int32_t* sv = sel.i32();
        int step = F > 1 ? sv[Q] - sv[0] : 1;
        for (int f = 0; f < F; f++)
            for (int q = 0; q < Q; q++)
                if (sv[f * Q + q] != f * step + q) return P.fail("front-end: GATHER selector is not a sliding window");
        fm->F = F; fm->hop = step * sub; fm->L = Q * sub;
        P.absorbed[pi] = 1;
        t = P.skip_up(ga.inputs[0]);
    }
    if (fm->window.empty()) fm->window.assign(fm->L, 1.0f);
    if ((int)fm->window.size() != fm->L) return P.fail("front-end: window length != frame length");
    if (fm->L > fm->Lfft) return P.fail("front-end: frame length > fft length");

    // optional zero padding of the whole clip ([1, n] -> [1, pad_left + n + pad_right])
    if (P.producer[t] >= 0 && m.ops[P.producer[t]].code == OP_PAD) {
        const TflOp& pd = m.ops[P.producer[t]];
        const TflTensor& pv = P.T(pd.inputs[1]);
        const auto& ish = P.T(pd.inputs[0]).shape;
        if (!pv.data || pv.numel() != 4 || ish.size() != 2 || pv.i32()[0] != 0 || pv.i32()[1] != 0 || pv.i32()[2] < 0 || pv.i32()[3] < 0)
            return P.fail("front-end: clip PAD must be constant [[0,0],[left,right]] on a [1, n] tensor");
        fm->pad_left = pv.i32()[2]; fm->pad_right = pv.i32()[3];
        P.absorbed[P.producer[t]] = 1;
        t = P.skip_up(pd.inputs[0]);
    }
    // normalisation: MUL(SUB(DIV(SUB(x, REDUCE_MIN x), ADD(REDUCE_MAX(.), eps)), c_sub), c_mul) - or none at all
    if (t == m.inputs[0]) {
        fm->normalize = false;
    } else {
        int p_mul = P.producer[t];
        if (p_mul < 0 || m.ops[p_mul].code != OP_MUL) return P.fail("front-end: normalisation (MUL) not found");
        int n2 = P.bin_const(m.ops[p_mul], &fm->norm_mul);
        if (n2 < 0) return P.fail("front-end: normalisation MUL needs a scalar constant");
        int p_sub = P.producer[n2];
        bool rhs = false;
        // (x - c), or the (x + (-c)) a converter may rewrite it to
        if (p_sub < 0 || (m.ops[p_sub].code != OP_SUB && m.ops[p_sub].code != OP_ADD)) return P.fail("front-end: normalisation (SUB c) not found");
        int nm = P.bin_const(m.ops[p_sub], &fm->norm_sub, &rhs);
        if (nm < 0 || (m.ops[p_sub].code == OP_SUB && !rhs)) return P.fail("front-end: normalisation SUB needs a scalar constant rhs");
        if (m.ops[p_sub].code == OP_ADD) fm->norm_sub = -fm->norm_sub;
        int p_div = P.producer[nm];
        if (p_div < 0 || m.ops[p_div].code != OP_DIV) return P.fail("front-end: normalisation (DIV) not found");
        int s1 = m.ops[p_div].inputs[0], dn = m.ops[p_div].inputs[1];
        int p_add = P.producer[dn];
        if (p_add < 0 || m.ops[p_add].code != OP_ADD) return P.fail("front-end: normalisation (ADD eps) not found");
        int mx = P.bin_const(m.ops[p_add], &fm->eps);
        if (mx < 0) return P.fail("front-end: normalisation ADD needs a scalar constant");
        int p_max = P.producer[mx];
        if (p_max < 0 || m.ops[p_max].code != OP_REDUCE_MAX || m.ops[p_max].inputs[0] != s1)
            return P.fail("front-end: normalisation (REDUCE_MAX of shifted signal) not found");
        int p_s1 = P.producer[s1];
        if (p_s1 < 0 || m.ops[p_s1].code != OP_SUB) return P.fail("front-end: normalisation (SUB min) not found");
        int x = m.ops[p_s1].inputs[0], mn = m.ops[p_s1].inputs[1];
        int p_min = P.producer[mn];
        if (p_min < 0 || m.ops[p_min].code != OP_REDUCE_MIN || m.ops[p_min].inputs[0] != x)
            return P.fail("front-end: normalisation (REDUCE_MIN) not found");
        if (x != m.inputs[0]) return P.fail("front-end: normalisation does not start at the graph input");
        for (int op : {p_mul, p_sub, p_div, p_add, p_max, p_s1, p_min}) P.absorbed[op] = 1;
    }

    // ---- downstream: real part -> mel matmul -> POW(s) -> REVERSE -> TRANSPOSE -> [1, n_mels, F, 1]
    t = P.skip_down(R.outputs[0]);
    int ci = P.only_consumer(t);
    if (ci < 0) return P.fail("front-end: STFT output must have one consumer");
    if (m.ops[ci].code == OP_COMPLEX_ABS) fm->magnitude = true;
    else if (!(m.ops[ci].code == OP_CAST || m.ops[ci].code == OP_REAL)) return P.fail("front-end: expected CAST/REAL/COMPLEX_ABS after RFFT2D");
    t = P.take(ci);
    ci = P.only_consumer(t);
    if (ci < 0 || (m.ops[ci].code != OP_FULLY_CONNECTED && m.ops[ci].code != OP_BATCH_MATMUL))
        return P.fail("front-end: mel projection (FULLY_CONNECTED / BATCH_MATMUL) not found");
    {
        const TflOp& fc = m.ops[ci];
        if (!P.is_const(fc.inputs[1]) || (fc.inputs.size() > 2 && fc.inputs[2] >= 0))
            return P.fail("front-end: mel projection must have constant weights and no bias");
        const TflTensor& w = P.T(fc.inputs[1]);
        const int nbins = fm->Lfft / 2 + 1;
        // FULLY_CONNECTED keeps [n_mels, bins]; tf.tensordot may also arrive as BATCH_MATMUL with the [bins, n_mels] matrix
        // (or its transpose with adj_y) on the right
        const bool bmm = fc.code == OP_BATCH_MATMUL;
        if (bmm && fc.adj_x) return P.fail("front-end: mel BATCH_MATMUL with adj_x is not supported");
        const bool rows_are_mels = !bmm || fc.adj_y;
        if (w.shape.size() != 2 || w.shape[rows_are_mels ? 1 : 0] != nbins || w.type != TT_FLOAT32)
            return P.fail("front-end: mel matrix shape mismatch");
        fm->n_mels = w.shape[rows_are_mels ? 0 : 1];
        if (rows_are_mels) fm->mel_tensor = fc.inputs[1];
        else {                                              // re-lay [bins, n_mels] -> [n_mels, bins]
            std::vector<float> wt((size_t)fm->n_mels * nbins);
            for (int k = 0; k < nbins; k++)
                for (int mm = 0; mm < fm->n_mels; mm++) wt[(size_t)mm * nbins + k] = w.f32()[(size_t)k * fm->n_mels + mm];
            fm->mel_tensor = const_cast<TflModel&>(m).add_const_f32(w.name + "/T", {fm->n_mels, nbins}, wt);
        }
        t = P.take(ci);
    }
    // log compression: MUL(LOG(MAXIMUM(x, floor)), scale)
    ci = P.only_consumer(t);
    if (ci >= 0 && m.ops[ci].code == OP_MAXIMUM) {
        int src = P.bin_const(m.ops[ci], &fm->log_floor);
        if (src < 0 || !(fm->log_floor > 0.f)) return P.fail("front-end: log compression needs MAXIMUM with a positive scalar floor");
        t = P.take(ci);
        ci = P.only_consumer(t);
        if (ci < 0 || m.ops[ci].code != OP_LOG) return P.fail("front-end: LOG after MAXIMUM not found");
        t = P.take(ci);
        fm->log_compress = true;
        ci = P.only_consumer(t);
        if (ci >= 0 && m.ops[ci].code == OP_MUL && P.bin_const(m.ops[ci], &fm->log_scale) >= 0) {
            t = P.take(ci);
        } else fm->log_scale = 1.f;
    }
    int npow = 0;
    // the square may arrive as POW(x, 2), SQUARE(x) or MUL(x, x)
    if (!fm->log_compress) {
        ci = P.only_consumer(t);
        const bool mul_self = ci < 0 && P.consumers[t].size() == 2 && P.consumers[t][0] == P.consumers[t][1] &&
                              m.ops[P.consumers[t][0]].code == OP_MUL && m.ops[P.consumers[t][0]].inputs[0] == t && m.ops[P.consumers[t][0]].inputs[1] == t;
        if (mul_self) ci = P.consumers[t][0];
        if (ci >= 0 && (m.ops[ci].code == OP_SQUARE || mul_self)) {
            fm->p1 = 2.0f; npow = 1;
            t = P.take(ci);
        }
    }
    while (!fm->log_compress && (ci = P.only_consumer(t)) >= 0 && m.ops[ci].code == OP_POW && npow < 2) {
        float e;
        if (!P.const_scalar(m.ops[ci].inputs[1], &e)) return P.fail("front-end: POW exponent must be a scalar constant");
        (npow == 0 ? fm->p1 : fm->p2) = e;
        npow++;
        t = P.take(ci);
    }
    ci = P.only_consumer(t);
    if (ci >= 0 && m.ops[ci].code == OP_REVERSE_V2) {
        const TflTensor& ax = P.T(m.ops[ci].inputs[1]);
        int rank = (int)P.T(m.ops[ci].inputs[0]).shape.size();
        if (!ax.data || ax.numel() != 1 || ((ax.i32()[0] + rank) % rank) != rank - 1)
            return P.fail("front-end: REVERSE_V2 must flip the mel axis");
        fm->reverse = true;
        t = P.take(ci);
        ci = P.only_consumer(t);
    }
    {
        // time-major image: the [1, F, n_mels] tensor is only reshaped to [1, F, n_mels, 1]
        const auto& ts = P.T(t).shape;
        if (!fm->reverse && ts.size() == 4 && ts[0] == 1 && ts[1] == fm->F && ts[2] == fm->n_mels && ts[3] == 1) {
            fm->time_major = true;
            fm->out_tensor = t;
            return true;
        }
    }
    if (ci < 0 || m.ops[ci].code != OP_TRANSPOSE) return P.fail("front-end: TRANSPOSE to [mel, time] not found");
    {
        const TflTensor& pm = P.T(m.ops[ci].inputs[1]);
        if (!pm.data || pm.numel() != 3 || pm.i32()[0] != 0 || pm.i32()[1] != 2 || pm.i32()[2] != 1)
            return P.fail("front-end: unsupported TRANSPOSE permutation");
        t = P.take(ci);
    }
    const auto& os = P.T(t).shape;
    if (os.size() != 4 || os[0] != 1 || os[1] != fm->n_mels || os[2] != fm->F || os[3] != 1)
        return P.fail("front-end: unexpected spectrogram tensor shape");
    fm->out_tensor = t;
    return true;
}

// G[n][m'] = sum_k cos(2 pi k n / Lfft) * Mel[k][m]   (fp64; the window is applied separately in fp32); krows: the bins with
// any non-zero mel weight (DFT truncation)
std::vector<double> build_G(const Planner& P, const FrontendMatch& fm, const std::vector<int>& krows, int Kp, int NTP) {
    const int nb = fm.Lfft / 2 + 1, nm = fm.n_mels, N = fm.Lfft;
    const float* melT = P.T(fm.mel_tensor).f32();      // [n_mels][nbins]
    std::vector<double> ctab(N);
    for (int i = 0; i < N; i++) ctab[i] = std::cos(2.0 * M_PI * (double)i / (double)N);
    std::vector<double> melk(krows.size() * (size_t)nm);
    for (size_t r = 0; r < krows.size(); r++)
        for (int mm = 0; mm < nm; mm++) melk[r * nm + mm] = (double)melT[(size_t)mm * nb + krows[r]];
    std::vector<double> G((size_t)Kp * NTP, 0.0);     // rows n' = 0..Lfft/2 (cos symmetry folds the rest)
    std::vector<double> row(nm);
    for (int n = 0; n <= fm.Lfft / 2; n++) {
        std::fill(row.begin(), row.end(), 0.0);
        for (size_t r = 0; r < krows.size(); r++) {
            double c = ctab[(size_t)(((long long)krows[r] * n) % N)];
            const double* mk = &melk[r * nm];
            for (int mm = 0; mm < nm; mm++) row[mm] += c * mk[mm];
        }
        for (int mo = 0; mo < nm; mo++) {
            int mm = fm.reverse ? nm - 1 - mo : mo;
            G[(size_t)n * NTP + mo] = row[mm];
        }
    }
    return G;
}

// Plan-time environment switches, read once at the top of Engine::build (the BNHIP_PW_* bits travel as Engine::pw_sw)
struct PlanSwitches {
    bool mel_banded = !getenv("BNHIP_NO_MEL_BANDED");      // banded mel matrices take k_mel_banded (else GEMM + k_mel_finish)
    bool fuse_mel = getenv("BNHIP_FUSE_MEL") != nullptr;    // opt-in: the banded mel inside the STFT kernel
    bool fuse_expdw = !(getenv("BNHIP_NO_FUSE_EXPDW") && atoi(getenv("BNHIP_NO_FUSE_EXPDW")) != 0);   // expand / stem + depthwise
    bool conv_igemm = !getenv("BNHIP_NO_CONV_IGEMM");      // real convolutions as implicit GEMMs
    bool stem_mfma = !getenv("BNHIP_NO_STEM_MFMA");        // MFMA image of the stem (needed by the stem fusion)
    bool fuse_stem = !getenv("BNHIP_NO_FUSE_STEM");        // stem + depthwise
};

// fused activation of a conv / dense op -> activation the kernels apply; the two the fused kernels do not implement
// (RELU_N1_TO_1, TANH) become a separate elementwise step (*post)
int map_act(int fused, int* post = nullptr) {
    if (post) *post = 0;
    switch (fused) {
        case 0: return ACT_NONE; case 1: return ACT_RELU; case 3: return ACT_RELU6;
        case 2: if (post) { *post = U_RELU_N1_TO_1; return ACT_NONE; } return -1;
        case 4: if (post) { *post = U_TANH; return ACT_NONE; } return -1;
        default: return -1;
    }
}

// top / left zero padding of a convolution-like op (SAME: TF's rule; VALID: none; explicit: folded-in PAD)
void conv_pads(const TflOp& o, int H, int W, int Ho, int Wo, int kh, int kw, int* pt, int* pl) {
    *pt = 0; *pl = 0;
    if (o.explicit_pad) { *pt = o.pad_t; *pl = o.pad_l; return; }
    if (o.padding == 0) {
        *pt = std::max((Ho - 1) * o.stride_h + (kh - 1) * o.dil_h + 1 - H, 0) / 2;
        *pl = std::max((Wo - 1) * o.stride_w + (kw - 1) * o.dil_w + 1 - W, 0) / 2;
    }
}

// shape -> rank-5 (batch + 4) by left-padding with 1s; false when the rank is larger or the leading dim is not 1
bool shape5(const std::vector<int>& sh, int out[5]) {
    std::vector<int> v = sh;
    while (v.size() > 5 && v[0] == 1) v.erase(v.begin());
    if (v.size() > 5) return false;
    for (int k = 0; k < 5; k++) out[k] = 1;
    for (size_t k = 0; k < v.size(); k++) out[5 - v.size() + k] = v[k];
    return out[0] == 1;
}

void dense_strides(const int d5[5], long st[5]) { st[4] = 1; for (int k = 3; k >= 0; k--) st[k] = st[k + 1] * d5[k + 1]; }

bool has_bias(const TflOp& o) { return o.inputs.size() > 2 && o.inputs[2] >= 0; }

// a strided view of the input, copied out densely: counts d[4], input strides sa[4] and offset (all per clip)
void copy_view(Step* s, const int d[4], const long sa[4], long offa) {
    long so = 1;
    for (int k = 3; k >= 0; k--) { s->g.d[k] = d[k]; s->g.sa[k] = sa[k]; s->g.so[k] = so; so *= d[k]; }
    s->g.offa = offa;
}

struct DwMatch { int di = -1, k = 0, s = 1, H = 0, W = 0, Ho = 0, Wo = 0, pt = 0, pl = 0, act = ACT_NONE; };   // Lowering::match_dw

// Plan-time state of one Engine::build: lowers the graph into the engine's steps / values / front-end specs and the host image
// of the weight arena.  Every refusal goes through fail(), which records the message and BNHIP_E_* code build() returns.
struct Lowering {
    Engine& E;
    TflModel& m;
    Planner P;
    const PlanSwitches sw;
    std::vector<Step>& steps;
    std::vector<Value>& vals;
    std::vector<FrontSpec>& specs;
    WeightPlan w;                        // weight arena image + per-step offsets into it
    std::map<int, size_t> wcache;        // tflite tensor -> offset (plain upload)
    std::map<int, int> tv;               // tflite tensor -> value id
    struct ScaledAlias { int v_data; int v_scale; };
    std::map<int, ScaledAlias> scaled;   // tflite tensor (SE MUL output) -> (data value, scale value)
    std::string err;
    int code = BNHIP_E_UNSUPPORTED;
    // front-end
    std::vector<FrontendMatch> fms;
    std::vector<int> chan_of;            // fms[i] -> channel of the spectrogram image
    int spec_tensor = -1, v_spec = -1;
    int v_xn = -1;                       // normalised clip (FFT front-end only)
    struct FftFin { int v_bins, spec; size_t o_mel, o_span; bool banded; bool fused; };
    std::vector<FftFin> fft_fin;         // FFT-path channels awaiting mel + pow + NHWC store

    Lowering(Engine& e, TflModel& mm, const PlanSwitches& s)
        : E(e), m(mm), P(mm), sw(s), steps(e.steps), vals(e.vals), specs(e.specs) {}

    bool fail(const std::string& msg, int c = BNHIP_E_UNSUPPORTED) { err = msg; code = c; return false; }

    // ---- weight image
    size_t wpush(const float* src, size_t n) {
        size_t off = align_up(w.img.size(), 64);       // 256-byte alignment
        w.img.resize(off + n);
        memcpy(&w.img[off], src, n * sizeof(float));
        return off;
    }
    size_t wpush(const std::vector<float>& v) { return wpush(v.data(), v.size()); }
    size_t wpush_bx(const std::vector<uint16_t>& img) {     // split-bf16 image, padded to whole floats
        std::vector<float> asf((img.size() + 1) / 2);
        memcpy(asf.data(), img.data(), img.size() * 2);
        return wpush(asf);
    }
    size_t wpush_i32(const std::vector<int>& v) { return wpush(reinterpret_cast<const float*>(v.data()), v.size()); }   // int32 image
    size_t wconst(int t) {
        auto it = wcache.find(t);
        if (it != wcache.end()) return it->second;
        size_t off = wpush(m.tensors[t].f32(), m.tensors[t].numel());
        wcache[t] = off;
        return off;
    }
    size_t wbias(const TflOp& o) { return has_bias(o) ? wconst(o.inputs[2]) : SIZE_MAX; }

    // ---- values and steps
    int new_val(int tfl, size_t elems) {
        Value v; v.tfl = tfl; v.elems = elems;
        vals.push_back(v);
        return (int)vals.size() - 1;
    }
    int out_val(int tfl, size_t elems) { int v = new_val(tfl, elems); tv[tfl] = v; return v; }
    int need_val(int t) const {
        auto it = tv.find(t);
        return it == tv.end() ? -1 : it->second;
    }
    // value of activation tensor t in *v; without one, fails with "<what>: input has no value<at>"
    bool input(int t, int* v, const std::string& what, const std::string& at = "") {
        *v = need_val(t);
        return *v >= 0 || fail(what + ": input has no value" + at);
    }
    bool add_step(const Step& s, size_t o0 = SIZE_MAX, size_t o1 = SIZE_MAX, size_t o2 = SIZE_MAX, size_t o3 = SIZE_MAX) {
        steps.push_back(s);
        w.step_w[0].push_back(o0); w.step_w[1].push_back(o1); w.step_w[2].push_back(o2); w.step_w[3].push_back(o3);
        size_t obx = SIZE_MAX;
        if (E.bf16x3 && s.kind == S_PW && o0 != SIZE_MAX && pw_bx3_ok(s.C)) {
            // three exact bf16 pieces of every weight, in the kernel's slab / lane order (1.5x the fp32 bytes)
            obx = wpush_bx(pw_bx3_image(&w.img[o0], s.Co, s.C));
            // WHICH arithmetic a layer runs is decided here, by shape, never by a timing (with a create-time race
            // between the two kernels the same clip could get different logits on different devices of one handle, and
            // from process to process): the split-bf16 kernel where the layer is compute-bound - algorithmic intensity at
            // max_batch >= 12 flop/B; measured at batch 256 the split wins every layer above that line by 19-32 % and ties
            // (+-4 %) the HBM-bound early projections below it (b1-b3: 5-10 flop/B) - everywhere with bf16x3 = 2 or
            // "precision":"bf16".  The autotuner then only picks the TILE inside that kernel family.
            const double Mr = (double)E.max_batch * s.H * s.W, Nr = s.Co, Kr = s.C;
            const double intensity = 2.0 * Mr * Nr * Kr / (4.0 * (Mr * Kr + Mr * Nr + Nr * Kr));
            if (E.bf16x3 >= 2 || E.precision == 1 || intensity >= 12.0) { steps.back().bx = 1; steps.back().wm = steps.back().wm_full = 6; }
        }
        w.step_bx.push_back(obx);
        return true;
    }
    // binds the step's output to TFLite tensor `outt` and appends it; a fused activation the kernels do not implement
    // (post != 0) runs as a separate elementwise step on an internal value
    bool emit(Step st, int outt, size_t elems, int post, size_t o0 = SIZE_MAX, size_t o1 = SIZE_MAX, size_t o2 = SIZE_MAX,
              size_t o3 = SIZE_MAX) {
        if (!post) { st.out = out_val(outt, elems); return add_step(st, o0, o1, o2, o3); }
        st.out = new_val(-1, elems);
        add_step(st, o0, o1, o2, o3);
        Step u; u.kind = S_EW_UNARY; u.kclass = "elementwise"; u.name = st.name + "/act"; u.in0 = st.out; u.op = post;
        u.out = out_val(outt, elems); u.bytes = 8.0 * elems;
        return add_step(u);
    }
    // a dense layer on k_pw_gemm: rows x K activations times an N x K weight matrix
    static Step gemm_step(const std::string& name, int in0, int rows, int K, int N, int act) {
        Step s; s.kind = S_PW; s.kclass = "pw_gemm"; s.name = name; s.in0 = in0;
        s.H = rows; s.W = 1; s.C = K; s.Ho = rows; s.Wo = 1; s.Co = N; s.act = act;
        s.flops = 2.0 * rows * K * N; s.bytes = 4.0 * rows * (K + N); s.wbytes = 4.0 * K * N;
        return s;
    }
    bool hwc(int t, int* H, int* W, int* C) const {
        const auto& s = m.tensors[t].shape;
        if (s.size() == 4 && s[0] == 1) { *H = s[1]; *W = s[2]; *C = s[3]; return true; }
        if (s.size() == 2 && s[0] == 1) { *H = 1; *W = 1; *C = s[1]; return true; }
        return false;
    }
    // trailing swish / sigmoid detection on tensor y produced by op `oi`; returns final tensor and act
    int trailing_act(int y, int* act) {
        if (P.consumers[y].size() == 2 && P.uses[y] == 2) {
            int a = P.consumers[y][0], b = P.consumers[y][1];
            int lg = m.ops[a].code == OP_LOGISTIC ? a : (m.ops[b].code == OP_LOGISTIC ? b : -1);
            int mu = lg == a ? b : a;
            if (lg >= 0 && m.ops[mu].code == OP_MUL && m.ops[mu].act == 0) {
                int sgt = m.ops[lg].outputs[0];
                const auto& mi = m.ops[mu].inputs;
                bool ok = P.uses[sgt] == 1 && ((mi[0] == y && mi[1] == sgt) || (mi[1] == y && mi[0] == sgt));
                if (ok) { P.absorbed[lg] = 1; P.absorbed[mu] = 1; *act = ACT_SWISH; return m.ops[mu].outputs[0]; }
            }
        } else if (P.uses[y] == 1 && P.consumers[y].size() == 1 && !P.absorbed[P.consumers[y][0]]) {
            // a stand-alone activation op right behind the producer (ONNX lowerings, unfused exports)
            const int ci = P.consumers[y][0];
            const int cc = m.ops[ci].code;
            const int a = cc == OP_LOGISTIC ? ACT_SIGMOID : cc == OP_RELU ? ACT_RELU : cc == OP_RELU6 ? ACT_RELU6 :
                          cc == OP_HARD_SWISH ? ACT_HARD_SWISH : -1;
            if (a >= 0) { P.absorbed[ci] = 1; *act = a; return m.ops[ci].outputs[0]; }
        }
        return y;
    }
    // an operand of a generic op: activation value, or constant uploaded to the weight arena
    struct Operand { int val = -1; size_t woff = SIZE_MAX; bool ok = false; };
    Operand operand(int t) {
        Operand r;
        if (t < 0) return r;
        r.val = need_val(t);
        if (r.val >= 0) { r.ok = true; return r; }
        if (P.is_const(t) && m.tensors[t].type == TT_FLOAT32) { r.woff = wconst(t); r.ok = true; }
        return r;
    }

    // ---- stages
    bool input_values() {
        const TflTensor& tin = m.tensors[m.inputs[0]];
        if (tin.type != TT_FLOAT32 || tin.shape.size() < 2 || tin.shape[0] != 1 || tin.numel() == 0 || tin.numel() > ((size_t)1 << 30))
            return fail("graph input must be float32 [1, ...] (one clip / one feature row per batch entry)");
        E.n_samples = (int)tin.numel();      // [1, n_samples] for the audio models; any [1, ...] block for generic graphs
        E.v_input = out_val(m.inputs[0], E.n_samples);
        vals[E.v_input].external = true;
        E.v_mm = new_val(-1, 2);
        return true;
    }
    // Every RFFT2D branch and the concat that stacks them into the spectrogram image.  Graphs without an STFT are accepted when
    // they are plain dense stacks on a [1,D] input: the bat heads (CustomClassifier, internal/inference/backend.go:31-52) and the
    // range-filter meta-model (RangeFilter, :55-76).
    bool match_frontends() {
        for (int i = 0; i < (int)m.ops.size(); i++)
            if (m.ops[i].code == OP_RFFT2D) {
                FrontendMatch fm;
                if (!match_frontend(P, i, &fm)) return fail(P.err);
                fms.push_back(fm);
            }
        chan_of.assign(fms.size(), 0);
        if (!fms.empty()) {
            int cc = P.only_consumer(fms[0].out_tensor);
            if (fms.size() == 1 && (cc < 0 || m.ops[cc].code != OP_CONCATENATION)) {
                spec_tensor = fms[0].out_tensor;
            } else {
                if (cc < 0 || m.ops[cc].code != OP_CONCATENATION || m.ops[cc].axis != 3)
                    return fail("front-end: spectrogram channels must be concatenated on axis 3");
                const TflOp& cat = m.ops[cc];
                if (cat.inputs.size() != fms.size()) return fail("front-end: concat arity != number of STFT branches");
                for (size_t i = 0; i < fms.size(); i++) {
                    auto it = std::find(cat.inputs.begin(), cat.inputs.end(), fms[i].out_tensor);
                    if (it == cat.inputs.end()) return fail("front-end: STFT branch does not feed the concat");
                    chan_of[i] = (int)(it - cat.inputs.begin());
                }
                P.absorbed[cc] = 1;
                spec_tensor = cat.outputs[0];
            }
        }
        E.C_spec = (int)fms.size();
        for (auto& fm : fms)
            if (fm.n_mels != fms[0].n_mels || fm.F != fms[0].F) return fail("front-end: branches disagree on [mel, time] shape");
        return true;
    }
    bool frontend() {
        if (fms.empty()) return true;
        for (auto& fm : fms)
            if (fm.normalize != fms[0].normalize || fm.pad_left != fms[0].pad_left || fm.pad_right != fms[0].pad_right)
                return fail("front-end: branches disagree on normalisation / clip padding");
        if (fms[0].normalize) {
            Step s; s.kind = S_MINMAX; s.name = "clip_minmax"; s.kclass = "clip_minmax"; s.in0 = E.v_input; s.out = E.v_mm;
            s.bytes = (double)E.n_samples * 4;
            add_step(s);
        }
        v_spec = out_val(spec_tensor, (size_t)fms[0].n_mels * fms[0].F * E.C_spec);
        for (int i = 0; i < (int)fms.size(); i++)
            if (!frontend_channel(i)) return false;
        mel_finish();
        return true;
    }
    // one STFT branch: its FrontSpec, then the FFT path (stft.hip) or the folded-GEMM kernel
    bool frontend_channel(int i) {
        const FrontendMatch& fm = fms[i];
        FrontSpec fs;
        fs.L = fm.L; fs.Lfft = fm.Lfft; fs.hop = fm.hop; fs.F = fm.F; fs.n_mels = fm.n_mels; fs.c = chan_of[i];
        fs.NTP = (int)align_up(fm.n_mels, 16);
        fs.Kp = (int)align_up(fm.Lfft / 2 + 1, frontend_kc(fm.Lfft, fm.hop, fs.NTP));
        if (fs.NTP > 128) return fail("front-end: more than 128 mel bins unsupported");
        if (fm.eps != fms[0].eps || fm.norm_sub != fms[0].norm_sub || fm.norm_mul != fms[0].norm_mul)
            return fail("front-end: branches use different normalisation constants");
        fs.p1 = fm.p1; fs.p2 = fm.p2; fs.eps = fm.eps; fs.norm_sub = fm.norm_sub; fs.norm_mul = fm.norm_mul;
        fs.normalize = fm.normalize; fs.log_compress = fm.log_compress; fs.time_major = fm.time_major;
        fs.pad_left = fm.pad_left; fs.log_floor = fm.log_floor; fs.log_scale = fm.log_scale;
        if ((long)(fm.F - 1) * fm.hop + fm.L > (long)E.n_samples + fm.pad_left + fm.pad_right)
            return fail("front-end: the framing selector reaches beyond the (padded) clip", BNHIP_E_MODEL);
        if (fm.time_major != fms[0].time_major) return fail("front-end: branches disagree on the image layout");
        // bins the mel matrix actually uses (DFT truncation)
        std::vector<int> bins;
        const int nbins = fm.Lfft / 2 + 1;
        const float* melT = P.T(fm.mel_tensor).f32();
        for (int k = 0; k < nbins; k++) {
            bool nz = false;
            for (int mm = 0; mm < fm.n_mels && !nz; mm++) nz = melT[(size_t)mm * nbins + k] != 0.0f;
            if (nz) bins.push_back(k);
        }
        const bool can_fft = stft_supported(fm.Lfft, (int)bins.size()) && !bins.empty();
        if (fm.magnitude && !can_fft) return fail("front-end: magnitude STFT (COMPLEX_ABS) is only implemented for fft_length 512 / 1024 / 2048");
        // the folded-GEMM kernel only knows the v2.4 layer (normalised clip, power compression, [mel, time] image)
        const bool variant = !fm.normalize || fm.log_compress || fm.time_major || fm.pad_left || fm.pad_right;
        if (variant && !can_fft)
            return fail("front-end: log-mel / unnormalised / padded front-ends are only implemented for fft_length 512 / 1024 / 2048");
        fs.fft = fm.magnitude || variant || (E.frontend_fft != 0 && can_fft);     // measured faster than the folded GEMM (0.95 vs 1.05 ms)
        if (fs.fft) return fft_channel(i, fs, bins);
        if (frontend_lds_bytes(fs.Lfft, fs.Kp, fs.hop, fs.NTP) > 160 * 1024) return fail("front-end: frame tile does not fit in LDS");
        return gemm_channel(i, fs, bins);
    }
    // normalise (once) -> STFT bins -> mel GEMM -> pow + NHWC store; the mel half is left to mel_finish()
    bool fft_channel(int i, FrontSpec fs, const std::vector<int>& bins) {
        const FrontendMatch& fm = fms[i];
        if (!fm.normalize) v_xn = E.v_input;
        if (v_xn < 0) {
            v_xn = new_val(-1, E.n_samples);
            Step nz; nz.kind = S_NORMALIZE; nz.name = "normalize"; nz.kclass = "frontend"; nz.in0 = E.v_input; nz.in1 = E.v_mm;
            nz.out = v_xn; nz.bytes = (double)E.n_samples * 8;
            add_step(nz);
        }
        fs.nb = (int)bins.size(); fs.nbp = (int)align_up(fs.nb, 4); fs.mode = fm.magnitude ? 1 : 0;
        const int nbins = fm.Lfft / 2 + 1;
        const float* melT = P.T(fm.mel_tensor).f32();
        std::vector<float> melw((size_t)fm.n_mels * fs.nbp, 0.f);                // [n_mels][nbp], rows in output order
        for (int mo = 0; mo < fm.n_mels; mo++) {
            int mm = fm.reverse ? fm.n_mels - 1 - mo : mo;
            for (int r = 0; r < fs.nb; r++) melw[(size_t)mo * fs.nbp + r] = melT[(size_t)mm * nbins + bins[r]];
        }
        const size_t o_win = wpush(fm.window), o_bins = wpush_i32(bins);
        const size_t o_mel = wpush(melw);
        std::vector<double> twt = stft_build_tables(fm.Lfft, bins.data(), fs.nb);
        fs.stft_zmask = stft_zmask(fm.Lfft, bins.data(), fs.nb);
        const size_t o_tw = wpush(reinterpret_cast<const float*>(twt.data()), twt.size() * 2);   // fp64 image, 256-B aligned
        specs.push_back(fs);
        const int si = (int)specs.size() - 1;
        // band structure of the mel rows: [lo, hi) of the nonzero columns.  A filterbank (2 nonzeros per bin) takes the
        // banded kernel; anything denser than a quarter of the matrix stays a GEMM.
        std::vector<int> span((size_t)2 * fm.n_mels, 0);
        long span_sum = 0;
        for (int mo = 0; mo < fm.n_mels; mo++) {
            int lo = fs.nb, hi = 0;
            for (int r = 0; r < fs.nb; r++)
                if (melw[(size_t)mo * fs.nbp + r] != 0.0f) { lo = std::min(lo, r); hi = r + 1; }
            if (hi == 0) lo = 0;
            span[2 * mo] = lo; span[2 * mo + 1] = hi;
            span_sum += hi - lo;
        }
        const size_t o_span = wpush_i32(span);
        const bool banded = sw.mel_banded && span_sum * 4 <= (long)fm.n_mels * fs.nb;
        // a banded mel matrix is applied by the wave that transformed the frame (k_stft_bins<.., MEL>): no bins tensor,
        // no separate mel kernel; the image value is written by the STFT step itself
        int mel_quads = 0;
        std::vector<float> meltab;
        // OPT-IN (BNHIP_FUSE_MEL=1): measured slower than the separate banded kernel in every form tried - the STFT kernels
        // are fp64-VALU / LDS-latency bound at two to three waves per SIMD, and the epilogue's extra LDS round trips land on
        // their critical path: v2.4 batch 256, stft0 440 -> 512-531 us, stft1 209 -> 293-320 us against the 116 us
        // k_mel_banded launch they replace (70.2 k -> 67.6-68.4 k clips/s).  It does remove 0.9 MB per clip of HBM traffic
        // and a launch, and stays parity-tested.
        if (banded && sw.fuse_mel) meltab = stft_mel_table(fm.Lfft, melw.data(), span.data(), fm.n_mels, fs.nb, fs.nbp, &mel_quads);
        const bool fused = !meltab.empty();
        int v_bins = fused ? -1 : new_val(-1, (size_t)fm.F * fs.nbp);
        Step st; st.kind = S_STFT; st.name = "stft" + std::to_string(i); st.kclass = "stft"; st.in0 = v_xn; st.out = fused ? v_spec : v_bins;
        st.spec = si;
        st.flops = (double)fm.F * 2.5 * fm.Lfft * std::log2((double)fm.Lfft / 2);      // ~5 N/2 log2(N/2) per frame
        st.bytes = (double)E.n_samples * 4 + (double)fm.F * (fused ? fm.n_mels : fs.nbp) * 4;
        if (fused) { st.mode = 1; st.S = mel_quads; st.name += "+mel"; st.flops += 4.0 * fm.F * fs.nb; }
        add_step(st, o_win, o_bins, o_tw, fused ? wpush(meltab) : SIZE_MAX);
        fft_fin.push_back({v_bins, si, o_mel, o_span, banded, fused});
        return true;
    }
    // the folded DFT x mel GEMM on the raw clip (k_frontend_gemm): real-part graphs whose fft length the FFT path does not take
    bool gemm_channel(int i, FrontSpec fs, const std::vector<int>& bins) {
        const FrontendMatch& fm = fms[i];
        std::vector<double> G = build_G(P, fm, bins, fs.Kp, fs.NTP);
        const size_t goff = wpush(reinterpret_cast<const float*>(G.data()), G.size() * 2);   // fp64 image, 256-B aligned
        // w[n'] for n' = 0..Lfft/2, then the mirror weights w[Lfft-n'] (0 when n' = 0, n' = Lfft/2, or beyond the frame)
        std::vector<float> wpad((size_t)2 * fs.Kp, 0.0f);
        for (int n = 0; n <= fm.Lfft / 2; n++) {
            if (n < fm.L) wpad[n] = fm.window[n];
            int mi = fm.Lfft - n;
            if (n > 0 && mi != n && mi < fm.L) wpad[fs.Kp + n] = fm.window[mi];
        }
        const size_t woff = wpush(wpad);
        specs.push_back(fs);
        Step f; f.kind = S_FRONTEND; f.name = "melspec" + std::to_string(i); f.kclass = "frontend";
        f.in0 = E.v_input; f.in1 = E.v_mm; f.out = v_spec; f.spec = (int)specs.size() - 1;
        f.flops = 2.0 * fm.F * (fm.Lfft / 2 + 1) * fm.n_mels;
        f.bytes = (double)E.n_samples * 4 + (double)fm.F * fm.n_mels * 4;
        return add_step(f, goff, woff);
    }
    // mel + pow + NHWC store of the FFT-path channels: two adjacent channels go out as one float2 per pixel.  Banded mel
    // matrices take one fused kernel; otherwise the mel projection is a k_pw_gemm per channel followed by k_mel_finish.
    void mel_finish() {
        for (size_t k = 0; k < fft_fin.size();) {
            if (fft_fin[k].fused) { k++; continue; }        // mel + compression + store happened in the STFT kernel
            const FrontSpec& a = specs[fft_fin[k].spec];
            const FrontSpec* b = k + 1 < fft_fin.size() && !fft_fin[k + 1].fused ? &specs[fft_fin[k + 1].spec] : nullptr;
            const bool pair = b && b->c == a.c + 1 && (a.c & 1) == 0 && b->F == a.F && b->n_mels == a.n_mels &&
                              b->log_compress == a.log_compress && b->log_floor == a.log_floor && b->log_scale == a.log_scale;
            const int nch = pair ? 2 : 1;
            const bool banded = fft_fin[k].banded && (!pair || fft_fin[k + 1].banded) && mel_banded_supported(a.n_mels, a.nbp, pair ? b->nbp : 0);
            if (banded) {
                Step mb; mb.kind = S_MELBAND; mb.name = "melband" + std::to_string(a.c); mb.kclass = "frontend";
                mb.in0 = fft_fin[k].v_bins; mb.spec = fft_fin[k].spec; mb.out = v_spec; mb.S = nch;
                double bytes = 4.0 * a.F * (a.nbp + a.n_mels), flops = 0;
                if (pair) {
                    mb.in1 = fft_fin[k + 1].v_bins; mb.op = fft_fin[k + 1].spec; mb.name += "+" + std::to_string(a.c + 1);
                    bytes += 4.0 * a.F * (specs[mb.op].nbp + a.n_mels);
                }
                for (int c = 0; c < nch; c++) flops += 4.0 * a.F * specs[fft_fin[k + c].spec].nb;     // ~2 nonzeros per bin
                mb.bytes = bytes; mb.flops = flops;
                add_step(mb, fft_fin[k].o_mel, fft_fin[k].o_span, pair ? fft_fin[k + 1].o_mel : SIZE_MAX, pair ? fft_fin[k + 1].o_span : SIZE_MAX);
                k += nch;
                continue;
            }
            int v_T[2] = {-1, -1};
            for (int c = 0; c < nch; c++) {
                const FrontSpec& fc = specs[fft_fin[k + c].spec];
                v_T[c] = new_val(-1, (size_t)fc.F * fc.n_mels);
                Step g = gemm_step("mel" + std::to_string(fc.c), fft_fin[k + c].v_bins, fc.F, fc.nbp, fc.n_mels, ACT_NONE);
                g.out = v_T[c];
                add_step(g, fft_fin[k + c].o_mel);
            }
            Step mf; mf.kind = S_MELFIN; mf.name = "melspec" + std::to_string(a.c); mf.kclass = "frontend";
            mf.in0 = v_T[0]; mf.spec = fft_fin[k].spec; mf.out = v_spec;
            mf.S = nch;
            if (pair) { mf.in1 = v_T[1]; mf.op = fft_fin[k + 1].spec; mf.name += "+" + std::to_string(a.c + 1); }
            mf.bytes = 8.0 * a.F * a.n_mels * mf.S;
            add_step(mf);
            k += mf.S;
        }
    }
    bool ops() {
        for (int oi = 0; oi < (int)m.ops.size(); oi++)
            if (!P.absorbed[oi] && !lower(m.ops[oi], m.tensors[m.ops[oi].outputs[0]].name)) return false;
        return true;
    }
    bool lower(const TflOp& o, const std::string& oname) {     // one function per op family
        switch (o.code) {
            case OP_CONV_2D: return conv2d(o, oname);
            case OP_DEPTHWISE_CONV_2D: return depthwise(o, oname);
            case OP_MEAN: return mean(o, oname);
            case OP_FULLY_CONNECTED: return fully_connected(o, oname);
            case OP_BATCH_MATMUL: return batch_matmul(o, oname);
            case OP_LOGISTIC: case OP_RELU: case OP_RELU6: case OP_HARD_SWISH:
            case OP_TANH: case OP_EXP: case OP_LOG: case OP_SQRT: case OP_RSQRT: case OP_ABS: case OP_NEG: case OP_SQUARE:
            case OP_LEAKY_RELU: case OP_ELU: case OP_SIN: case OP_COS: case OP_FLOOR: case OP_CEIL: case OP_ROUND:
            case OP_RELU_N1_TO_1: case OP_GELU: return unary(o, oname);
            case OP_ADD: case OP_MUL: case OP_SUB: case OP_DIV: case OP_POW: case OP_MAXIMUM: case OP_MINIMUM:
            case OP_SQUARED_DIFFERENCE: return binary(o, oname);
            case OP_AVERAGE_POOL_2D: case OP_MAX_POOL_2D: return pool(o, oname);
            case OP_SOFTMAX: return softmax(o, oname);
            case OP_CONCATENATION: return concat(o, oname);
            case OP_STRIDED_SLICE: case OP_SLICE: return slice(o, oname);
            case OP_TRANSPOSE: case OP_REVERSE_V2: return transpose(o, oname);
            case OP_GATHER: return gather(o, oname);
            case OP_PAD: case OP_PADV2: return pad(o, oname);
            case OP_SPLIT: return split(o, oname);
            case OP_SUM: case OP_REDUCE_MAX: case OP_REDUCE_MIN: case OP_REDUCE_PROD: return reduce(o, oname);
            case OP_RESHAPE: case OP_SQUEEZE: case OP_EXPAND_DIMS: case OP_CAST: return reshape(o, oname);
            default: return fail(std::string("unsupported operator ") + op_name(o.code) + " (code " + std::to_string(o.code) + ") at " + oname);
        }
    }
    bool bind_outputs() {
        auto it = tv.find(m.outputs[0]);
        if (it == tv.end()) return fail("graph output 0 was not produced by a supported op");
        E.v_logits = it->second;
        E.n_classes = (int)vals[E.v_logits].elems;
        vals[E.v_logits].external = true;
        if (m.outputs.size() > 1) {
            auto ie = tv.find(m.outputs[1]);
            if (ie == tv.end()) return fail("graph output 1 (embedding) was not produced by a supported op");
            E.v_emb = ie->second;
            E.emb_dim = (int)vals[E.v_emb].elems;
        }
        return true;
    }

    // ---- op families
    bool conv2d(const TflOp& o, const std::string& oname) {
        const int in_t = o.inputs[0];
        if (!P.is_const(o.inputs[1])) return fail("CONV_2D with non-constant filter");
        const TflTensor& wt = m.tensors[o.inputs[1]];
        int H, W, C, Ho, Wo, Co;
        if (!hwc(in_t, &H, &W, &C) || !hwc(o.outputs[0], &Ho, &Wo, &Co) || wt.shape.size() != 4 || wt.shape[3] != C)
            return fail("CONV_2D: unsupported shapes at " + oname);
        const int kh = wt.shape[1], kw = wt.shape[2];
        int post = 0;
        int act = map_act(o.act, &post);
        if (act < 0) return fail("CONV_2D: unsupported fused activation");
        int outt = o.outputs[0];
        if (act == ACT_NONE && !post) outt = trailing_act(outt, &act);
        const size_t boff = wbias(o);
        const bool pw = kh == 1 && kw == 1 && o.stride_h == 1 && o.stride_w == 1 && !o.explicit_pad && Ho == H && Wo == W;
        const bool se_scaled = scaled.find(in_t) != scaled.end();
        Step s; s.name = oname; s.H = H; s.W = W; s.C = C; s.Ho = Ho; s.Wo = Wo; s.Co = Co; s.act = act;
        // ---- MBConv front half: 1x1 expand whose only consumer is a depthwise conv -> one fused kernel
        DwMatch d;
        if (pw && !post && sw.fuse_expdw && !se_scaled && match_dw(outt, &d) &&
            expdw_supported(d.k, d.s, C, Co, act, E.bf16x3 ? E.precision : 0) &&
            expdw_sum_slabs(ExpDwGeo{d.k, d.s, d.H, d.W, d.Ho, d.Wo, d.pt, d.pl}) > 0 && need_val(in_t) >= 0) {
            Step f = s;
            f.name = oname + "+dw"; f.in0 = need_val(in_t);
            f.flops = 2.0 * H * W * C * Co + 2.0 * d.Ho * d.Wo * Co * d.k * d.k;
            f.bytes = 4.0 * ((double)H * W * C + (double)d.Ho * d.Wo * Co);
            f.wbytes = 4.0 * (C * Co + d.k * d.k * Co);
            emit_expand_dw(f, d, wt.f32(), C, C, expdw_kw(C), has_bias(o) ? m.tensors[o.inputs[2]].f32() : nullptr);
            if (E.bf16x3 && expdw_bx_ok(C)) {          // split-bf16 image of the expand weights (autotuned per layer)
                w.step_bx.back() = wpush_bx(expdw_bx_image(wt.f32(), Co, C));
                // (arithmetic by rule, not by timing: the split-bf16 phase 1 measured +0-0.5 % at best, so it is
                // used only where asked for)
                if (E.bf16x3 >= 2 || E.precision == 1) steps.back().bx = 1;
            }
            return true;
        }
        if (pw) {
            s.kind = S_PW; s.kclass = "pw_gemm";
            auto sc = scaled.find(in_t);
            if (sc != scaled.end()) { s.in0 = sc->second.v_data; s.in1 = sc->second.v_scale; }
            else s.in0 = need_val(in_t);
            if (s.in0 < 0) return fail("CONV_2D: input has no value: " + oname);
            // residual ADD fusion
            if (!post && P.uses[outt] == 1 && P.consumers[outt].size() == 1) {
                int ai = P.consumers[outt][0];
                const TflOp& ad = m.ops[ai];
                if (ad.code == OP_ADD && ad.act == 0 && !P.absorbed[ai]) {
                    int other = ad.inputs[0] == outt ? ad.inputs[1] : ad.inputs[0];
                    int vo = need_val(other);
                    if (vo >= 0 && m.tensors[other].shape == m.tensors[outt].shape) {
                        s.in2 = vo; P.absorbed[ai] = 1; outt = ad.outputs[0];
                    }
                }
            }
            s.flops = 2.0 * H * W * C * Co;
            s.bytes = 4.0 * ((double)H * W * C + (double)H * W * Co * (s.in2 >= 0 ? 2 : 1));
            s.wbytes = 4.0 * C * Co;
            return emit(s, outt, (size_t)Ho * Wo * Co, post, wconst(o.inputs[1]), boff);
        }
        const bool igemm = conv_igemm_supported(C, Co, kh, kw) && !se_scaled && sw.conv_igemm &&
                           (double)E.max_batch * Ho * Wo * std::max(Ho * Wo, C) < 1.0e12;
        if (!igemm && o.dil_h == 1 && o.dil_w == 1 && !(Co & 3)) return conv_direct(o, oname, s, outt, post, boff);
        if (igemm) {
            // a real convolution (kh x kw over >= 4 input channels): implicit GEMM on the f32 MFMA, weights as in the file
            s.kind = S_CONV_IGEMM; s.kclass = "conv_igemm";
        } else {
            // dilated convolutions and channel counts the vectorised kernels do not cover: generic kernel, weights as
            // in the file (OHWI)
            s.kind = S_CONV_GENERIC; s.kclass = "conv_generic";
            if (se_scaled) return fail("CONV_2D: squeeze-excite scale in front of an unsupported convolution at " + oname);
        }
        if (!input(in_t, &s.in0, "CONV_2D", ": " + oname)) return false;
        s.kh = kh; s.kw = kw; s.sh = o.stride_h; s.sw = o.stride_w; s.g.dh = o.dil_h; s.g.dw = o.dil_w;
        conv_pads(o, H, W, Ho, Wo, kh, kw, &s.pt, &s.pl);
        s.flops = 2.0 * Ho * Wo * Co * kh * kw * C;
        s.bytes = 4.0 * ((double)H * W * C + (double)Ho * Wo * Co);
        if (igemm) s.wbytes = 4.0 * kh * kw * C * Co;
        return emit(s, outt, (size_t)Ho * Wo * Co, post, wconst(o.inputs[1]), boff);
    }
    // direct convolution (the stem), with the MFMA stem image where the shape allows it and the stem + depthwise fusion behind it
    bool conv_direct(const TflOp& o, const std::string& oname, Step s, int outt, int post, size_t boff) {
        const int H = s.H, W = s.W, C = s.C, Ho = s.Ho, Wo = s.Wo, Co = s.Co;
        const TflTensor& wt = m.tensors[o.inputs[1]];
        const int kh = wt.shape[1], kw = wt.shape[2];
        s.kind = S_CONV_DIRECT; s.kclass = "conv_direct";
        if (scaled.find(o.inputs[0]) != scaled.end()) return fail("CONV_2D: squeeze-excite scale in front of an unsupported convolution at " + oname);
        if (!input(o.inputs[0], &s.in0, "CONV_2D", ": " + oname)) return false;
        s.kh = kh; s.kw = kw; s.sh = o.stride_h; s.sw = o.stride_w;
        conv_pads(o, H, W, Ho, Wo, kh, kw, &s.pt, &s.pl);
        // re-lay OHWI -> [kh][kw][Cin][Cout]
        std::vector<float> wr((size_t)kh * kw * C * Co);
        const float* ws = wt.f32();
        for (int oc = 0; oc < Co; oc++)
            for (int i = 0; i < kh; i++)
                for (int j = 0; j < kw; j++)
                    for (int ic = 0; ic < C; ic++)
                        wr[(((size_t)i * kw + j) * C + ic) * Co + oc] = ws[(((size_t)oc * kh + i) * kw + j) * C + ic];
        s.flops = 2.0 * Ho * Wo * Co * kh * kw * C;
        s.bytes = 4.0 * ((double)H * W * C + (double)Ho * Wo * Co);
        const ConvParams cp{nullptr, nullptr, nullptr, nullptr, 1, H, W, C, Ho, Wo, Co, kh, kw, s.sh, s.sw, s.pt, s.pl, s.act};
        if (!stem_mfma_supported(cp) || !sw.stem_mfma) {
            return emit(s, outt, (size_t)Ho * Wo * Co, post, wpush(wr), boff);
        }
        // second image for the MFMA stem: [Cout][32], kk = i*8 + j*2 + ic
        std::vector<float> wm((size_t)Co * 32, 0.f), bp(Co, 0.f);
        for (int oc = 0; oc < Co; oc++)
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++)
                    for (int ic = 0; ic < 2; ic++)
                        wm[(size_t)oc * 32 + i * 8 + j * 2 + ic] = ws[(((size_t)oc * kh + i) * kw + j) * C + ic];
        if (has_bias(o)) memcpy(bp.data(), m.tensors[o.inputs[2]].f32(), (size_t)Co * sizeof(float));
        // ---- stem whose only consumer is a 3x3 stride-1 depthwise conv: one k_expand_dw<STEM> launch; the stem output (the
        // largest tensor of the network) never reaches HBM
        DwMatch d;
        if (!post && sw.fuse_expdw && sw.fuse_stem && (Co % 32) == 0 && match_dw(outt, &d) && d.s == 1 && d.k == 3 &&
            expdw_sum_slabs(ExpDwGeo{d.k, 1, d.H, d.W, d.Ho, d.Wo, d.pt, d.pl, true}) > 0) {
            Step f = s;
            f.name = oname + "+dw"; f.mode = 1;
            f.H = Ho; f.W = Wo; f.C = 32;
            f.H2 = H; f.W2 = W; f.pt2 = s.pt; f.pl2 = s.pl;
            f.flops = 2.0 * Ho * Wo * Co * kh * kw * C + 2.0 * d.Ho * d.Wo * Co * d.k * d.k;
            f.bytes = 4.0 * ((double)H * W * C + (double)d.Ho * d.Wo * Co);
            f.wbytes = 4.0 * (Co * 32 + d.k * d.k * Co);
            // expand-side weights: the first 24 of the 32 columns of the MFMA stem image (row 2 is the 8-wide half slab of the
            // fused kernel; columns 24..31 are the zero padding of k_stem_mfma)
            emit_expand_dw(f, d, wm.data(), 32, 24, 24, bp.data());
            return true;
        }
        const size_t o_wr = wpush(wr), o_wm = wpush(wm), o_bp = wpush(bp);
        return emit(s, outt, (size_t)Ho * Wo * Co, post, o_wr, boff, o_wm, o_bp);
    }
    // The only consumer of tensor t is a depthwise conv k_expand_dw can run as its second half (constant square filter, no
    // multiplier / dilation, equal strides, a kernel activation); the callers add their own stride / filter / tile conditions.
    bool match_dw(int t, DwMatch* d) {
        if (P.uses[t] != 1 || P.consumers[t].size() != 1) return false;
        const int di = P.consumers[t][0];
        const TflOp& o = m.ops[di];
        int C, Co;
        if (o.code != OP_DEPTHWISE_CONV_2D || P.absorbed[di] || o.inputs[0] != t || !P.is_const(o.inputs[1]) ||
            !hwc(t, &d->H, &d->W, &C) || !hwc(o.outputs[0], &d->Ho, &d->Wo, &Co) || Co != C || o.depth_multiplier != 1 ||
            o.dil_h != 1 || o.dil_w != 1 || o.stride_h != o.stride_w)
            return false;
        const auto& ws = m.tensors[o.inputs[1]].shape;
        d->act = map_act(o.act);
        if (ws.size() != 4 || ws[1] != ws[2] || ws[3] != C || d->act < 0) return false;
        d->di = di; d->k = ws[1]; d->s = o.stride_h;
        conv_pads(o, d->H, d->W, d->Ho, d->Wo, d->k, d->k, &d->pt, &d->pl);
        return true;
    }
    // Appends k_expand_dw step f (expand half set by the caller), claiming the matched depthwise conv d and a trailing activation.
    // we: Co rows of `ld` floats, the first K used; be: expand bias or nullptr.  Every load in k_expand_dw is unconditional
    // (see expdw.hip): the parameters go in as padded copies [Cp][Kw], [Cp], [k*k][Cp], [Cp].
    void emit_expand_dw(Step f, const DwMatch& d, const float* we, int ld, int K, int Kw, const float* be) {
        const TflOp& dw = m.ops[d.di];
        int dout = dw.outputs[0], act_d = d.act;
        if (act_d == ACT_NONE) dout = trailing_act(dout, &act_d);
        P.absorbed[d.di] = 1;
        const int Co = f.Co, Cp = expdw_cp(Co), kk = d.k * d.k;
        f.kind = S_EXPAND_DW; f.kclass = "expand_dw";
        f.Ho = d.Ho; f.Wo = d.Wo; f.kh = d.k; f.kw = d.k; f.sh = d.s; f.sw = d.s; f.pt = d.pt; f.pl = d.pl; f.act2 = act_d;
        f.out = out_val(dout, (size_t)d.Ho * d.Wo * Co);
        std::vector<float> wep((size_t)Cp * Kw, 0.f), bep(Cp, 0.f), wdp((size_t)kk * Cp, 0.f), bdp(Cp, 0.f);
        for (int n = 0; n < Co; n++) memcpy(&wep[(size_t)n * Kw], we + (size_t)n * ld, (size_t)K * sizeof(float));
        if (be) memcpy(bep.data(), be, (size_t)Co * sizeof(float));
        const float* dsrc = m.tensors[dw.inputs[1]].f32();
        for (int t = 0; t < kk; t++) memcpy(&wdp[(size_t)t * Cp], dsrc + (size_t)t * Co, (size_t)Co * sizeof(float));
        if (has_bias(dw)) memcpy(bdp.data(), m.tensors[dw.inputs[2]].f32(), (size_t)Co * sizeof(float));
        const size_t o_we = wpush(wep), o_be = wpush(bep), o_wd = wpush(wdp), o_bd = wpush(bdp);
        add_step(f, o_we, o_be, o_wd, o_bd);
    }
    bool depthwise(const TflOp& o, const std::string& oname) {
        const int in_t = o.inputs[0];
        const TflTensor& wt = m.tensors[o.inputs[1]];
        int H, W, C, Ho, Wo, Co;
        if (!P.is_const(o.inputs[1]) || !hwc(in_t, &H, &W, &C) || !hwc(o.outputs[0], &Ho, &Wo, &Co) || wt.shape.size() != 4 ||
            wt.shape[3] != Co || o.depth_multiplier < 1 || Co != C * o.depth_multiplier)
            return fail("DEPTHWISE_CONV_2D: unsupported configuration at " + oname + " (filter must be constant [1,kh,kw,C*depth_multiplier])");
        int post = 0;
        int act = map_act(o.act, &post);
        if (act < 0) return fail("DEPTHWISE_CONV_2D: unsupported fused activation");
        int outt = o.outputs[0];
        if (act == ACT_NONE && !post) outt = trailing_act(outt, &act);
        Step s; s.name = oname;
        if (!input(in_t, &s.in0, "DEPTHWISE_CONV_2D")) return false;
        s.H = H; s.W = W; s.C = C; s.Ho = Ho; s.Wo = Wo; s.Co = Co; s.act = act;
        s.kh = wt.shape[1]; s.kw = wt.shape[2]; s.sh = o.stride_h; s.sw = o.stride_w;
        conv_pads(o, H, W, Ho, Wo, s.kh, s.kw, &s.pt, &s.pl);
        s.flops = 2.0 * Ho * Wo * Co * s.kh * s.kw;
        s.bytes = 4.0 * ((double)H * W * C + (double)Ho * Wo * Co);
        const size_t boff = wbias(o);
        if (o.depth_multiplier != 1 || o.dil_h != 1 || o.dil_w != 1) {
            // channel multipliers and dilation: generic kernel (out channel oc reads input channel oc / multiplier)
            s.kind = S_CONV_GENERIC; s.kclass = "conv_generic";
            s.g.dh = o.dil_h; s.g.dw = o.dil_w; s.g.depthwise = 1; s.g.mult = o.depth_multiplier;
        } else {
            s.kind = S_DW; s.kclass = "dwconv";
        }
        return emit(s, outt, (size_t)Ho * Wo * Co, post, wconst(o.inputs[1]), boff);
    }
    // spatial MEAN over [1, H, W, C]: per-slab partial sums (emitted by the producing depthwise / expand_dw step where it can),
    // then the squeeze-excite block it opens or a plain finish.  Any other MEAN is a generic reduction.
    bool mean(const TflOp& o, const std::string& oname) {
        const int in_t = o.inputs[0];
        int H, W, C;
        const TflTensor& ax = m.tensors[o.inputs[1]];
        const bool spatial = hwc(in_t, &H, &W, &C) && ax.data && ax.numel() == 2 &&
                             ((ax.i32()[0] == 1 && ax.i32()[1] == 2) || (ax.i32()[0] == 2 && ax.i32()[1] == 1));
        if (!spatial) return reduce(o, oname);
        int vin;
        if (!input(in_t, &vin, "MEAN")) return false;
        int S = mean_splits(H * W);
        bool fused_sum = false;
        Step mp; mp.kind = S_MEAN_PARTIAL; mp.kclass = "mean"; mp.name = oname + "/partial";
        mp.in0 = vin; mp.H = H; mp.W = W; mp.C = C;
        // a depthwise / expand_dw producer emits the per-slab channel sums itself; the partial buffer is sized for whichever tile
        // shape (or, for S_DW, the LDS-staged form with its own tile counts) the autotuner ends up with
        int slabs = 0, cap = 0;
        if (!steps.empty() && steps.back().kind == S_EXPAND_DW && steps.back().out == vin) {
            const Step& d = steps.back();
            // (not Engine::expdw_geo: no skw, because wbx is not bound yet; the eight-wave shapes it offers tile as their four-wave twins, so neither count depends on it)
            const ExpDwGeo dg{d.kh, d.sh, d.H, d.W, d.Ho, d.Wo, d.pt, d.pl, d.mode == 1};
            slabs = expdw_sum_slabs(dg);
            cap = expdw_max_slabs(dg);
        } else if (!steps.empty() && steps.back().kind == S_DW && steps.back().out == vin) {
            const Step& d = steps.back();
            const DwParams dp = dw_params(d);
            slabs = cap = dwconv_sum_slabs(dp);
            if (dwconv_lds_supported(dp)) cap = std::max(cap, expdw_max_slabs(ExpDwGeo{d.kh, d.sh, d.H, d.W, d.Ho, d.Wo, d.pt, d.pl}));
        }
        if (slabs > 0) {
            S = slabs;
            fused_sum = true;
            mp.out = new_val(-1, (size_t)cap * C);
            steps.back().out2 = mp.out;
            steps.back().S = S;
        }
        mp.S = S;
        if (!fused_sum) mp.out = new_val(-1, (size_t)S * C);
        mp.bytes = 4.0 * H * W * C;
        if (squeeze_excite(o, vin, mp, fused_sum)) return true;
        if (!fused_sum) add_step(mp);
        Step mf; mf.kind = S_MEAN_FINISH; mf.kclass = "mean"; mf.name = oname;
        mf.in0 = mp.out; mf.H = H; mf.W = W; mf.C = C; mf.S = S;
        mf.out = out_val(o.outputs[0], (size_t)C);
        return add_step(mf);
    }
    // op oi: [*, K] -> [*, N] with constant weights (a 1x1 CONV_2D or a FULLY_CONNECTED)?
    bool fc_like(int oi, int K, int* N) const {
        if (oi < 0 || P.absorbed[oi]) return false;
        const TflOp& f = m.ops[oi];
        if ((f.code != OP_CONV_2D && f.code != OP_FULLY_CONNECTED) || f.inputs.size() < 2 || !P.is_const(f.inputs[1])) return false;
        const TflTensor& wt = m.tensors[f.inputs[1]];
        if (wt.type != TT_FLOAT32) return false;
        if (f.code == OP_CONV_2D) {
            if (wt.shape.size() != 4 || wt.shape[1] != 1 || wt.shape[2] != 1 || wt.shape[3] != K || f.stride_h != 1 || f.stride_w != 1) return false;
        } else if (wt.shape.size() != 2 || wt.shape[1] != K) return false;
        if (has_bias(f) && (!P.is_const(f.inputs[2]) || (int)m.tensors[f.inputs[2]].numel() != wt.shape[0])) return false;
        *N = wt.shape[0];
        return true;
    }
    // activation of FC op oi (fused, or trailing); returns the tensor after it, -1 for an activation the kernels lack
    int fc_act(int oi, int* act) {
        *act = map_act(m.ops[oi].act);
        if (*act < 0) return -1;
        int y = m.ops[oi].outputs[0];
        if (*act == ACT_NONE) y = trailing_act(y, act);
        return y;
    }
    // MEAN -> FC(Cr) + act -> FC(C) + act -> MUL with the MEAN's input, each FC a 1x1 CONV_2D or a FULLY_CONNECTED, with any
    // pure reshapes in between (Keras: GlobalAveragePooling2D -> Reshape(1,1,C) -> Conv2D ... -> Multiply).  False (and the
    // graph view as it was): no such block behind this MEAN.
    bool squeeze_excite(const TflOp& o, int vin, const Step& mp, bool fused_sum) {
        const int in_t = o.inputs[0], mt = o.outputs[0], H = mp.H, W = mp.W, C = mp.C;
        if (P.uses[mt] != 1) return false;
        const std::vector<char> save = P.absorbed;
        auto no = [&] { P.absorbed = save; return false; };
        int c1 = P.only_consumer(P.skip_down(mt));
        int Cr = 0, Cb = 0;
        if (!fc_like(c1, C, &Cr)) return no();
        if (!se_supported(C, Cr)) return no();       // k_se's LDS request would exceed a launch's limit: the generic steps run the block
        int act1 = ACT_NONE, act2 = ACT_NONE;
        int r = fc_act(c1, &act1);
        if (r < 0) return no();
        r = P.skip_down(r);
        int c2 = P.uses[r] == 1 ? P.only_consumer(r) : -1;
        if (!fc_like(c2, Cr, &Cb) || Cb != C) return no();
        int e = fc_act(c2, &act2);
        if (e < 0) return no();
        e = P.skip_down(e);
        int mu = P.uses[e] == 1 ? P.only_consumer(e) : -1;
        if (mu < 0 || m.ops[mu].code != OP_MUL || m.ops[mu].act != 0) return no();
        int other = m.ops[mu].inputs[0] == e ? m.ops[mu].inputs[1] : m.ops[mu].inputs[0];
        if (other != in_t) return no();
        // matched
        P.absorbed[c1] = 1; P.absorbed[c2] = 1; P.absorbed[mu] = 1;
        if (!fused_sum) add_step(mp);
        Step ss; ss.kind = S_SE; ss.kclass = "se"; ss.name = m.tensors[mt].name + "/se";
        ss.in0 = mp.out; ss.H = H; ss.W = W; ss.C = C; ss.Cr = Cr; ss.S = mp.S; ss.act = act1; ss.act2 = act2;
        ss.out = out_val(e, (size_t)C);
        ss.flops = 4.0 * C * Cr;
        const size_t b1 = wbias(m.ops[c1]), b2 = wbias(m.ops[c2]);
        // second FC transposed [C][Cr] -> [Cr][C] so the kernel reads it coalesced
        std::vector<float> w2t((size_t)C * Cr);
        const float* w2s = m.tensors[m.ops[c2].inputs[1]].f32();
        for (int cc = 0; cc < C; cc++)
            for (int jj = 0; jj < Cr; jj++) w2t[(size_t)jj * C + cc] = w2s[(size_t)cc * Cr + jj];
        const size_t o_w1 = wconst(m.ops[c1].inputs[1]), o_w2 = wpush(w2t);
        add_step(ss, o_w1, b1, o_w2, b2);
        // the scale folds into a following 1x1 conv (k_pw_gemm reads it per input channel); otherwise an explicit MUL
        int u = m.ops[mu].outputs[0];
        int pc = P.uses[u] == 1 ? P.only_consumer(u) : -1;
        bool fold = false;
        if (pc >= 0 && m.ops[pc].code == OP_CONV_2D && P.is_const(m.ops[pc].inputs[1]) && m.ops[pc].inputs[0] == u) {
            const TflTensor& wp = m.tensors[m.ops[pc].inputs[1]];
            fold = wp.shape.size() == 4 && wp.shape[1] == 1 && wp.shape[2] == 1 && m.ops[pc].stride_h == 1 &&
                   m.ops[pc].stride_w == 1 && (C % 4) == 0;
        }
        if (fold) {
            scaled[u] = ScaledAlias{vin, ss.out};
        } else {
            Step bs; bs.kind = S_BINARY; bs.kclass = "elementwise"; bs.name = m.tensors[u].name;
            bs.in0 = vin; bs.in1 = ss.out; bs.op = 1; bs.mode = 1; bs.H = H; bs.W = W; bs.C = C;
            bs.out = out_val(u, (size_t)H * W * C); bs.bytes = 8.0 * H * W * C;
            add_step(bs);
        }
        return true;
    }
    bool fully_connected(const TflOp& o, const std::string& oname) {
        const int in_t = o.inputs[0];
        if (!P.is_const(o.inputs[1])) return fail("FULLY_CONNECTED: weights must be constant at " + oname);
        const TflTensor& wt = m.tensors[o.inputs[1]];
        const int C = wt.shape[1], N = wt.shape[0];
        const size_t in_elems = m.tensors[in_t].numel();
        if (C <= 0 || in_elems % (size_t)C) return fail("FULLY_CONNECTED: input size is not a multiple of the weight width at " + oname);
        const int rows = (int)(in_elems / (size_t)C);          // leading dimensions flatten into GEMM rows
        int post = 0;
        int act = map_act(o.act, &post);
        if (act < 0) return fail("FULLY_CONNECTED: unsupported fused activation");
        int outt = o.outputs[0];
        if (act == ACT_NONE && !post && std::find(m.outputs.begin(), m.outputs.end(), outt) == m.outputs.end())
            outt = trailing_act(outt, &act);
        int vin;
        if (!input(in_t, &vin, "FULLY_CONNECTED")) return false;
        const Step s = gemm_step(oname, vin, rows, C, N, act);
        const size_t boff = wbias(o);
        return emit(s, outt, (size_t)rows * N, post, wconst(o.inputs[1]), boff);
    }
    // activation x constant matrix only (a dense layer written as a matmul): W[N][K] = rhs^T at plan time
    bool batch_matmul(const TflOp& o, const std::string& oname) {
        const int in_t = o.inputs[0], r_t = o.inputs[1];
        if (!P.is_const(r_t) || m.tensors[r_t].shape.size() != 2 || o.adj_x) return fail("BATCH_MATMUL: only activation x constant [K,N] is supported at " + oname);
        const TflTensor& r = m.tensors[r_t];
        const int K = o.adj_y ? r.shape[1] : r.shape[0], N = o.adj_y ? r.shape[0] : r.shape[1];
        const size_t in_elems = m.tensors[in_t].numel();
        if (K <= 0 || in_elems % (size_t)K) return fail("BATCH_MATMUL: inner dimensions disagree at " + oname);
        std::vector<float> wt((size_t)N * K);
        for (int n = 0; n < N; n++)
            for (int k = 0; k < K; k++) wt[(size_t)n * K + k] = o.adj_y ? r.f32()[(size_t)n * K + k] : r.f32()[(size_t)k * N + n];
        const int rows = (int)(in_elems / (size_t)K);
        int vin;
        if (!input(in_t, &vin, "BATCH_MATMUL")) return false;
        return emit(gemm_step(oname, vin, rows, K, N, ACT_NONE), o.outputs[0], (size_t)rows * N, 0, wpush(wt));
    }
    // elementwise unary ops: the four the fused kernels' activations cover run as S_UNARY, the rest on the generic tier
    bool unary(const TflOp& o, const std::string& oname) {
        int vin;
        if (!input(o.inputs[0], &vin, op_name(o.code))) return false;
        Step s; s.kind = S_EW_UNARY; s.kclass = "elementwise"; s.name = oname; s.in0 = vin;
        switch (o.code) {
            case OP_LOGISTIC: s.kind = S_UNARY; s.act = ACT_SIGMOID; break; case OP_RELU: s.kind = S_UNARY; s.act = ACT_RELU; break;
            case OP_RELU6: s.kind = S_UNARY; s.act = ACT_RELU6; break; case OP_HARD_SWISH: s.kind = S_UNARY; s.act = ACT_HARD_SWISH; break;
            case OP_TANH: s.op = U_TANH; break; case OP_EXP: s.op = U_EXP; break; case OP_LOG: s.op = U_LOG; break;
            case OP_SQRT: s.op = U_SQRT; break; case OP_RSQRT: s.op = U_RSQRT; break; case OP_ABS: s.op = U_ABS; break;
            case OP_NEG: s.op = U_NEG; break; case OP_SQUARE: s.op = U_SQUARE; break; case OP_LEAKY_RELU: s.op = U_LEAKY_RELU; break;
            case OP_ELU: s.op = U_ELU; break; case OP_SIN: s.op = U_SIN; break; case OP_COS: s.op = U_COS; break;
            case OP_FLOOR: s.op = U_FLOOR; break; case OP_CEIL: s.op = U_CEIL; break; case OP_ROUND: s.op = U_ROUND; break;
            case OP_RELU_N1_TO_1: s.op = U_RELU_N1_TO_1; break;
            default: s.op = o.approximate ? U_GELU_TANH : U_GELU; break;
        }
        if (s.kind == S_EW_UNARY) s.g.alpha = o.alpha;
        s.out = out_val(o.outputs[0], vals[vin].elems); s.bytes = 8.0 * vals[vin].elems;
        return add_step(s);
    }
    // numpy-style broadcasting over right-aligned shapes; either operand may be a constant
    bool binary(const TflOp& o, const std::string& oname) {
        if (o.act < 0 || o.act > 4) return fail("binary op: unsupported fused activation");
        Operand A = operand(o.inputs[0]), B = operand(o.inputs[1]);
        if (!A.ok || !B.ok) return fail(std::string(op_name(o.code)) + ": operand has no value at " + oname);
        if (A.val < 0 && B.val < 0) return fail(std::string(op_name(o.code)) + ": constant expression (no activation operand) at " + oname);
        int da[5], db[5], dz[5];
        if (!shape5(m.tensors[o.inputs[0]].shape, da) || !shape5(m.tensors[o.inputs[1]].shape, db) || !shape5(m.tensors[o.outputs[0]].shape, dz))
            return fail("binary op: rank > 4 (+batch) unsupported at " + oname);
        for (int k = 0; k < 5; k++)
            if ((da[k] != dz[k] && da[k] != 1) || (db[k] != dz[k] && db[k] != 1)) return fail("binary op: shapes do not broadcast at " + oname);
        long sta[5], stb[5];
        dense_strides(da, sta); dense_strides(db, stb);
        Step s; s.kind = S_EW_BINARY; s.kclass = "elementwise"; s.name = oname; s.act = o.act;
        s.op = o.code == OP_ADD ? B_ADD : o.code == OP_MUL ? B_MUL : o.code == OP_SUB ? B_SUB : o.code == OP_DIV ? B_DIV :
               o.code == OP_POW ? B_POW : o.code == OP_MAXIMUM ? B_MAX : o.code == OP_MINIMUM ? B_MIN : B_SQDIFF;
        for (int k = 0; k < 4; k++) {
            s.g.d[k] = dz[k + 1];
            s.g.sa[k] = da[k + 1] == 1 ? 0 : sta[k + 1];
            s.g.sb[k] = db[k + 1] == 1 ? 0 : stb[k + 1];
        }
        s.in0 = A.val; s.in1 = B.val; s.g.a_const = A.val < 0; s.g.b_const = B.val < 0;
        const size_t elems = m.tensors[o.outputs[0]].numel();
        s.out = out_val(o.outputs[0], elems); s.bytes = 12.0 * elems;
        return add_step(s, A.woff, B.woff);
    }
    bool pool(const TflOp& o, const std::string& oname) {
        int H, W, C, Ho, Wo, Co;
        if (!hwc(o.inputs[0], &H, &W, &C) || !hwc(o.outputs[0], &Ho, &Wo, &Co) || Co != C || o.filter_h < 1 || o.filter_w < 1)
            return fail(std::string(op_name(o.code)) + ": unsupported shapes at " + oname);
        if (o.act < 0 || o.act > 4) return fail("pool: unsupported fused activation");
        int vin;
        if (!input(o.inputs[0], &vin, op_name(o.code))) return false;
        Step s; s.kind = S_POOL; s.kclass = "pool"; s.name = oname; s.in0 = vin; s.act = o.act;
        s.mode = o.code == OP_AVERAGE_POOL_2D ? 0 : 1;
        s.H = H; s.W = W; s.C = C; s.Ho = Ho; s.Wo = Wo; s.Co = C; s.kh = o.filter_h; s.kw = o.filter_w; s.sh = o.stride_h; s.sw = o.stride_w;
        if (o.padding == 0) {
            s.pt = std::max((Ho - 1) * s.sh + s.kh - H, 0) / 2;
            s.pl = std::max((Wo - 1) * s.sw + s.kw - W, 0) / 2;
        }
        s.out = out_val(o.outputs[0], (size_t)Ho * Wo * C); s.bytes = 4.0 * ((double)H * W * C + (double)Ho * Wo * C);
        return add_step(s);
    }
    bool softmax(const TflOp& o, const std::string& oname) {
        const int vin = need_val(o.inputs[0]);
        const auto& sh = m.tensors[o.inputs[0]].shape;
        if (vin < 0 || sh.empty()) return fail("SOFTMAX: input has no value");
        Step s; s.kind = S_SOFTMAX; s.kclass = "softmax"; s.name = oname; s.in0 = vin;
        s.C = sh.back(); s.H = (int)(vals[vin].elems / (size_t)std::max(s.C, 1)); s.g.alpha = o.beta;
        s.out = out_val(o.outputs[0], vals[vin].elems); s.bytes = 8.0 * vals[vin].elems;
        return add_step(s);
    }
    bool concat(const TflOp& o, const std::string& oname) {
        int dz[5];
        const int rank = (int)m.tensors[o.outputs[0]].shape.size();
        if (!shape5(m.tensors[o.outputs[0]].shape, dz) || rank < 1) return fail("CONCATENATION: rank unsupported at " + oname);
        int ax = o.axis < 0 ? o.axis + rank : o.axis;
        if (ax < 0 || ax >= rank) return fail("CONCATENATION: axis out of range at " + oname);
        const int ax5 = ax + (5 - std::min(rank, 5));
        if (ax5 < 1) return fail("CONCATENATION: cannot concatenate along the batch dimension at " + oname);
        if (o.act != 0) return fail("CONCATENATION: fused activation unsupported");
        long sto[5]; dense_strides(dz, sto);
        const int vout = out_val(o.outputs[0], m.tensors[o.outputs[0]].numel());
        long off = 0; int total_ax = 0;
        for (size_t ii = 0; ii < o.inputs.size(); ii++) {
            Operand A = operand(o.inputs[ii]);
            int di[5];
            if (!A.ok || !shape5(m.tensors[o.inputs[ii]].shape, di)) return fail("CONCATENATION: operand has no value at " + oname);
            for (int k = 0; k < 5; k++) if (k != ax5 && di[k] != dz[k]) return fail("CONCATENATION: operand shapes disagree at " + oname);
            long sti[5]; dense_strides(di, sti);
            Step s; s.kind = S_COPY; s.kclass = "copy"; s.name = oname + "/" + std::to_string(ii); s.in0 = A.val; s.out = vout;
            s.g.a_const = A.val < 0;
            for (int k = 0; k < 4; k++) { s.g.d[k] = di[k + 1]; s.g.sa[k] = sti[k + 1]; s.g.so[k] = sto[k + 1]; }
            s.g.offo = off * sto[ax5];
            s.bytes = 8.0 * m.tensors[o.inputs[ii]].numel();
            add_step(s, A.woff);
            off += di[ax5]; total_ax += di[ax5];
        }
        if (total_ax != dz[ax5]) return fail("CONCATENATION: operand sizes do not add up at " + oname);
        return true;
    }
    bool slice(const TflOp& o, const std::string& oname) {
        const std::string what = op_name(o.code);
        int vin;
        const auto& ish = m.tensors[o.inputs[0]].shape; const int rank = (int)ish.size();
        if (!input(o.inputs[0], &vin, what, " at " + oname)) return false;
        for (size_t k = 1; k < o.inputs.size(); k++)
            if (!P.is_const(o.inputs[k]) || (int)m.tensors[o.inputs[k]].numel() != rank)
                return fail(what + ": begin/end/strides must be constant vectors of the input rank at " + oname);
        if (o.code == OP_STRIDED_SLICE && (o.ellipsis_mask || o.new_axis_mask)) return fail("STRIDED_SLICE: ellipsis / new-axis masks unsupported at " + oname);
        int di[5];
        if (!shape5(ish, di) || rank > 5) return fail(what + ": rank unsupported at " + oname);
        const int lead = 5 - rank;
        long sti[5]; dense_strides(di, sti);
        int cnt5[5] = {1, 1, 1, 1, 1}; long st5[5] = {0, 0, 0, 0, 0}; long off = 0;
        const int32_t* bg = m.tensors[o.inputs[1]].i32();
        const int32_t* en = m.tensors[o.inputs[2]].i32();
        const int32_t* sr = o.code == OP_STRIDED_SLICE ? m.tensors[o.inputs[3]].i32() : nullptr;
        size_t total = 1;
        for (int k = 0; k < rank; k++) {
            const int dim = ish[k];
            long b, e, st;
            if (o.code == OP_SLICE) {                              // begin / size; size -1 = to the end
                b = bg[k]; st = 1; e = en[k] < 0 ? dim : b + en[k];
            } else {
                st = sr[k];
                if (st == 0) return fail("STRIDED_SLICE: zero stride at " + oname);
                b = bg[k]; e = en[k];
                if (b < 0) b += dim;
                if (e < 0) e += dim;
                if ((o.begin_mask >> k) & 1) b = st > 0 ? 0 : dim - 1;
                if ((o.end_mask >> k) & 1) e = st > 0 ? dim : -1;
                if ((o.shrink_axis_mask >> k) & 1) { e = b + 1; st = 1; }
                if (st > 0) { b = std::min<long>(std::max<long>(b, 0), dim); e = std::min<long>(std::max<long>(e, 0), dim); }
                else { b = std::min<long>(std::max<long>(b, -1), dim - 1); e = std::min<long>(std::max<long>(e, -1), dim - 1); }
            }
            long n = st > 0 ? (e > b ? (e - b + st - 1) / st : 0) : (b > e ? (b - e - st - 1) / (-st) : 0);
            if (n <= 0 || b < 0 || b >= dim || b + (n - 1) * st < 0 || b + (n - 1) * st >= dim) return fail(what + ": empty or out-of-range slice at " + oname);
            cnt5[lead + k] = (int)n; st5[lead + k] = st * sti[lead + k]; off += b * sti[lead + k];
            total *= (size_t)n;
        }
        if (cnt5[0] != 1 || total != m.tensors[o.outputs[0]].numel()) return fail(what + ": slice does not match the output shape at " + oname);
        Step s; s.kind = S_COPY; s.kclass = "copy"; s.name = oname; s.in0 = vin;
        copy_view(&s, cnt5 + 1, st5 + 1, off);
        s.out = out_val(o.outputs[0], total); s.bytes = 8.0 * total;
        return add_step(s);
    }
    bool transpose(const TflOp& o, const std::string& oname) {
        const int vin = need_val(o.inputs[0]);
        const auto& ish = m.tensors[o.inputs[0]].shape; const int rank = (int)ish.size();
        int di[5];
        if (vin < 0 || !P.is_const(o.inputs[1]) || !shape5(ish, di) || rank > 5) return fail(std::string(op_name(o.code)) + ": unsupported operands at " + oname);
        const int lead = 5 - rank;
        long sti[5]; dense_strides(di, sti);
        int dz[5]; long st5[5]; long off = 0;
        const TflTensor& pt = m.tensors[o.inputs[1]];
        if (o.code == OP_TRANSPOSE) {
            if ((int)pt.numel() != rank) return fail("TRANSPOSE: permutation length != rank at " + oname);
            int perm5[5]; std::vector<char> seen(5, 0);
            for (int k = 0; k < lead; k++) perm5[k] = k;
            for (int k = 0; k < rank; k++) { int pk = pt.i32()[k]; if (pk < 0 || pk >= rank) return fail("TRANSPOSE: bad permutation at " + oname); perm5[lead + k] = lead + pk; }
            for (int k = 0; k < 5; k++) { if (seen[perm5[k]]) return fail("TRANSPOSE: bad permutation at " + oname); seen[perm5[k]] = 1; }
            if (perm5[0] != 0) return fail("TRANSPOSE: the batch dimension cannot move at " + oname);
            for (int k = 0; k < 5; k++) { dz[k] = di[perm5[k]]; st5[k] = sti[perm5[k]]; }
        } else {
            for (int k = 0; k < 5; k++) { dz[k] = di[k]; st5[k] = sti[k]; }
            for (size_t q = 0; q < pt.numel(); q++) {
                int ax = pt.i32()[q]; if (ax < 0) ax += rank;
                if (ax < 0 || ax >= rank || lead + ax == 0) return fail("REVERSE_V2: bad axis at " + oname);
                off += (long)(di[lead + ax] - 1) * sti[lead + ax]; st5[lead + ax] = -sti[lead + ax];
            }
        }
        Step s; s.kind = S_COPY; s.kclass = "copy"; s.name = oname; s.in0 = vin;
        copy_view(&s, dz + 1, st5 + 1, off);
        s.out = out_val(o.outputs[0], vals[vin].elems); s.bytes = 8.0 * vals[vin].elems;
        return add_step(s);
    }
    // GATHER of an activation with a CONSTANT selector that is affine in its (<= 2) indices - tf.signal.frame's sliding window
    // idx[f][q] = f * step + q, a strided pick idx[i] = i0 + i * a, a single element - is a strided view of the input: one copy
    // kernel.  (Inside a recognised audio front-end the framing never runs: the STFT kernel fetches its frames from the clip;
    // this is the literal path for graphs the recogniser does not take.)
    bool gather(const TflOp& o, const std::string& oname) {
        const int vin = need_val(o.inputs[0]);
        const auto& ish = m.tensors[o.inputs[0]].shape; const int rank = (int)ish.size();
        if (vin < 0 || o.inputs.size() != 2 || !P.is_const(o.inputs[1]) || m.tensors[o.inputs[1]].type != TT_INT32 || o.batch_dims != 0)
            return fail("GATHER: needs an activation and a constant int32 selector at " + oname);
        const TflTensor& sel = m.tensors[o.inputs[1]];
        int ax = o.axis < 0 ? o.axis + rank : o.axis;
        if (ax < 1 || ax >= rank || sel.shape.size() > 2 || sel.numel() < 1) return fail("GATHER: unsupported axis / selector rank at " + oname);
        const int n0 = sel.shape.empty() ? 1 : sel.shape[0], n1 = sel.shape.size() == 2 ? sel.shape[1] : 1;
        const int32_t* sv = sel.i32();
        const long i0 = sv[0], a0 = n0 > 1 ? (long)sv[n1] - sv[0] : 0, a1 = n1 > 1 ? (long)sv[1] - sv[0] : 0;
        for (int f = 0; f < n0; f++)
            for (int q = 0; q < n1; q++) {
                const long want = i0 + f * a0 + q * a1;
                if (sv[(size_t)f * n1 + q] != want || want < 0 || want >= ish[ax]) return fail("GATHER: the constant selector is not affine (or out of range) at " + oname);
            }
        long pre = 1, post = 1;
        for (int k = 1; k < ax; k++) pre *= ish[k];
        for (int k = ax + 1; k < rank; k++) post *= ish[k];
        if (ish[0] != 1) return fail("GATHER: batch dimension must be 1 at " + oname);
        Step s; s.kind = S_COPY; s.kclass = "copy"; s.name = oname; s.in0 = vin;
        // view [pre, n0, n1, post] of the input [pre, ish[ax], post]
        const int din[4] = {(int)pre, n0, n1, (int)post};
        const long sin_[4] = {(long)ish[ax] * post, a0 * post, a1 * post, 1};
        copy_view(&s, din, sin_, i0 * post);
        const size_t elems = m.tensors[o.outputs[0]].numel();
        if ((size_t)(pre * n0 * n1 * post) != elems) return fail("GATHER: output shape mismatch at " + oname);
        s.out = out_val(o.outputs[0], elems); s.bytes = 8.0 * elems;
        return add_step(s);
    }
    bool pad(const TflOp& o, const std::string& oname) {
        const std::string what = op_name(o.code);
        const int vin = need_val(o.inputs[0]);
        const auto& ish = m.tensors[o.inputs[0]].shape; const int rank = (int)ish.size();
        int di[5], dz[5];
        if (vin < 0 || !P.is_const(o.inputs[1]) || (int)m.tensors[o.inputs[1]].numel() != 2 * rank || !shape5(ish, di) ||
            !shape5(m.tensors[o.outputs[0]].shape, dz) || rank > 5)
            return fail(what + ": unsupported operands at " + oname);
        float fillv = 0.0f;
        if (o.code == OP_PADV2 && !P.const_scalar(o.inputs[2], &fillv)) return fail("PADV2: pad value must be a scalar constant at " + oname);
        const int lead = 5 - rank;
        const int32_t* pv = m.tensors[o.inputs[1]].i32();
        long sto[5]; dense_strides(dz, sto);
        long off = 0;
        for (int k = 0; k < rank; k++) {
            if (pv[2 * k] < 0 || pv[2 * k + 1] < 0 || di[lead + k] + pv[2 * k] + pv[2 * k + 1] != dz[lead + k])
                return fail(what + ": paddings disagree with the output shape at " + oname);
            off += (long)pv[2 * k] * sto[lead + k];
        }
        if (dz[0] != 1) return fail(what + ": batch padding unsupported at " + oname);
        Step s; s.kind = S_COPY; s.kclass = "copy"; s.name = oname; s.in0 = vin;
        long si = 1;
        for (int k = 3; k >= 0; k--) { s.g.d[k] = di[k + 1]; s.g.sa[k] = si; si *= di[k + 1]; s.g.so[k] = sto[k + 1]; }
        s.g.offo = off; s.g.fill = true; s.g.alpha = fillv;
        const size_t elems = m.tensors[o.outputs[0]].numel();
        s.out = out_val(o.outputs[0], elems); s.bytes = 4.0 * (elems + vals[vin].elems);
        return add_step(s);
    }
    // inputs: axis (constant scalar), value; outputs: num_splits equal slices along the axis
    bool split(const TflOp& o, const std::string& oname) {
        const int vin = need_val(o.inputs[1]);
        const auto& ish = m.tensors[o.inputs[1]].shape; const int rank = (int)ish.size();
        int di[5];
        if (vin < 0 || !P.is_const(o.inputs[0]) || m.tensors[o.inputs[0]].numel() != 1 || !shape5(ish, di) || rank > 5) return fail("SPLIT: unsupported operands at " + oname);
        int ax = m.tensors[o.inputs[0]].i32()[0]; if (ax < 0) ax += rank;
        const int lead = 5 - rank, nsp = (int)o.outputs.size();
        if (ax < 0 || ax >= rank || lead + ax == 0 || nsp < 1 || di[lead + ax] % nsp) return fail("SPLIT: bad axis or split count at " + oname);
        long sti[5]; dense_strides(di, sti);
        int dz[5]; for (int k = 0; k < 5; k++) dz[k] = di[k];
        dz[lead + ax] = di[lead + ax] / nsp;
        size_t elems = 1; for (int k = 0; k < 5; k++) elems *= (size_t)dz[k];
        for (int q = 0; q < nsp; q++) {
            if (m.tensors[o.outputs[q]].numel() != elems) return fail("SPLIT: output shape mismatch at " + oname);
            Step s; s.kind = S_COPY; s.kclass = "copy"; s.name = m.tensors[o.outputs[q]].name; s.in0 = vin;
            copy_view(&s, dz + 1, sti + 1, (long)q * dz[lead + ax] * sti[lead + ax]);
            s.out = out_val(o.outputs[q], elems); s.bytes = 8.0 * elems;
            add_step(s);
        }
        return true;
    }
    // SUM / REDUCE_MAX / REDUCE_MIN / REDUCE_PROD, and the MEANs that are not a spatial average
    bool reduce(const TflOp& o, const std::string& oname) {
        const std::string what = op_name(o.code);
        const int vin = need_val(o.inputs[0]);
        const auto& ish = m.tensors[o.inputs[0]].shape; const int rank = (int)ish.size();
        int di[5];
        if (vin < 0 || !P.is_const(o.inputs[1]) || !shape5(ish, di) || rank > 5) return fail(what + ": unsupported operands at " + oname);
        const int lead = 5 - rank;
        const TflTensor& ax = m.tensors[o.inputs[1]];
        Step s; s.kind = S_REDUCE; s.kclass = "reduce"; s.name = oname; s.in0 = vin;
        for (size_t q = 0; q < ax.numel(); q++) {
            int a = ax.i32()[q]; if (a < 0) a += rank;
            if (a < 0 || a >= rank || lead + a == 0) return fail(what + ": bad axis at " + oname);
            s.g.mask |= 1 << (lead + a - 1);
        }
        size_t elems = 1;
        for (int k = 0; k < 4; k++) { s.g.d[k] = di[k + 1]; if (!((s.g.mask >> k) & 1)) elems *= (size_t)di[k + 1]; }
        if (elems != m.tensors[o.outputs[0]].numel()) return fail(what + ": output shape mismatch at " + oname);
        s.op = o.code == OP_MEAN ? R_MEAN : o.code == OP_SUM ? R_SUM : o.code == OP_REDUCE_MAX ? R_MAX : o.code == OP_REDUCE_MIN ? R_MIN : R_PROD;
        s.out = out_val(o.outputs[0], elems); s.bytes = 4.0 * (vals[vin].elems + elems);
        return add_step(s);
    }
    // RESHAPE / SQUEEZE / EXPAND_DIMS / float CAST: the output is a contiguous alias of the input value
    bool reshape(const TflOp& o, const std::string& oname) {
        int vin;
        if (!input(o.inputs[0], &vin, op_name(o.code))) return false;
        if (o.code == OP_CAST && (m.tensors[o.inputs[0]].type != TT_FLOAT32 || m.tensors[o.outputs[0]].type != TT_FLOAT32))
            return fail("CAST: only float32 -> float32 outside the recognised front-end at " + oname);
        if (m.tensors[o.outputs[0]].numel() != vals[vin].elems) return fail("reshape changes element count");
        tv[o.outputs[0]] = vin;
        return true;
    }
};

// ------------------------------------------------------------------------------------------------ plan-wide passes
// Which graph outputs are the logits and the embedding: the reference decides by model family from the input length and the
// number / size of the outputs (internal/inference/onnx/detection.go:24-112: v2.4 logits 0 [+ embedding 1]; BirdNET v3.0
// (160000 samples, 2 outputs) the 1280-wide port is the embedding, the other the predictions; Perch v2 (160000 samples, 4
// outputs: embedding, spatial embedding, spectrogram, logits) logits 3, embedding 0).  Explicit options (>= 0 / != -2) win.
// The boundary returns logits + embedding only, so every other output is dropped here and never computed.
bool select_outputs(TflModel& m, int* logits_output, int* embedding_output) {
    if (m.inputs.empty() || m.outputs.empty()) return true;
    const size_t n_in = m.tensors[m.inputs[0]].numel();
    const int n_out = (int)m.outputs.size();
    auto last_dim = [&](int oi) { const auto& sh = m.tensors[m.outputs[oi]].shape; return sh.empty() ? 0 : sh.back(); };
    int li = 0, ei = n_out > 1 ? 1 : -1;
    if (n_in == 160000 && n_out == 4) { li = 3; ei = 0; }
    else if (n_in == 160000 && n_out == 2) { if (last_dim(0) == 1280) { ei = 0; li = 1; } else { ei = 1; li = 0; } }
    if (*logits_output >= 0) li = *logits_output;
    if (*embedding_output != -2) ei = *embedding_output;
    if (li < 0 || li >= n_out || ei >= n_out || ei == li) return false;
    std::vector<int> keep = {m.outputs[li]};
    if (ei >= 0) keep.push_back(m.outputs[ei]);
    *logits_output = li; *embedding_output = ei;
    m.outputs = keep;
    return true;
}

// first / last step that touches each value
void mark_liveness(std::vector<Value>& vals, const std::vector<Step>& steps) {
    for (int si = 0; si < (int)steps.size(); si++) {
        for (int v : {steps[si].in0, steps[si].in1, steps[si].in2, steps[si].out, steps[si].out2}) {
            if (v < 0) continue;
            if (vals[v].first < 0) vals[v].first = si;
            vals[v].last = si;
        }
    }
}

// Best-fit placement of every internal value in an activation arena sized for `cap` clips, reusing the memory of values that
// are dead; writes Value::offset (or offset_lane for the lane layout) and returns the arena size.
size_t plan_arena(std::vector<Value>& vals, const std::vector<Step>& steps, size_t cap, bool lane_plan, bool no_reuse) {
    struct Block { size_t off, size; };
    std::vector<Block> free_list;
    size_t top = 0;
    auto off_of = [&](int v) -> size_t& { return lane_plan ? vals[v].offset_lane : vals[v].offset; };
    std::vector<std::vector<int>> born(steps.size() + 1), dies(steps.size() + 2);
    for (int v = 0; v < (int)vals.size(); v++) {
        if (vals[v].external || vals[v].first < 0) continue;
        born[vals[v].first].push_back(v);
        dies[std::min<size_t>(vals[v].last + 1, steps.size() + 1)].push_back(v);
    }
    for (size_t si = 0; si <= steps.size(); si++) {
        for (int v : dies[si]) {
            free_list.push_back(Block{off_of(v), align_up(vals[v].elems * 4 * cap, 256)});
            // coalesce
            std::sort(free_list.begin(), free_list.end(), [](const Block& a, const Block& b) { return a.off < b.off; });
            std::vector<Block> merged;
            for (auto& b : free_list) {
                if (!merged.empty() && merged.back().off + merged.back().size == b.off) merged.back().size += b.size;
                else merged.push_back(b);
            }
            free_list.swap(merged);
        }
        if (si == steps.size()) break;
        for (int v : born[si]) {
            size_t need = align_up(vals[v].elems * 4 * cap, 256);
            int best = -1;
            if (no_reuse) free_list.clear();
            for (int i = 0; i < (int)free_list.size(); i++)
                if (free_list[i].size >= need && (best < 0 || free_list[i].size < free_list[best].size)) best = i;
            if (best >= 0) {
                off_of(v) = free_list[best].off;
                free_list[best].off += need; free_list[best].size -= need;
                if (free_list[best].size == 0) free_list.erase(free_list.begin() + best);
            } else {
                // extend the arena top (absorb a trailing free block if adjacent)
                if (!free_list.empty() && free_list.back().off + free_list.back().size == top) {
                    off_of(v) = free_list.back().off;
                    top = off_of(v) + need;
                    free_list.pop_back();
                } else {
                    off_of(v) = top; top += need;
                }
            }
        }
    }
    return top;
}

}  // namespace

int pw_switches_from_env() {
    auto sw = [](const char* name, int off, int force) {
        const char* e = getenv(name);
        return !e ? 0 : e[0] == '0' ? off : e[0] == '2' ? force : 0;
    };
    return sw("BNHIP_PW_B16", PW_SW_B16_OFF, PW_SW_B16_FORCE) | sw("BNHIP_PW_B16S", PW_SW_B16S_OFF, PW_SW_B16S_FORCE) |
           sw("BNHIP_PW_WS", PW_SW_WS_OFF, PW_SW_WS_FORCE) | sw("BNHIP_PW_LAT", PW_SW_LAT_OFF, 0) |
           sw("BNHIP_PW_TAIL", PW_SW_TAIL_OFF, PW_SW_TAIL_FORCE);
}

// Which pointwise steps may run their consumer in the GEMM's epilogue (k_pw_b16's clip-aligned row tiles, PwTail): an fp32 engine's
// split-bf16 GEMM without scale or residual whose output is read by nothing but the next step's stride-1 SAME 3 x 3 / 5 x 5 depthwise
// convolution, or by the global spatial mean, with a clip's H W pixels a multiple of 16 that divides an offered row tile.  Whether
// the fused form is then used is the tuner's decision per layer (autotune_tail) and the call's size (tail_taken).
void Engine::mark_tails() {
    for (auto& s : steps) s.tail = 0;
    if (precision != 0 || (pw_sw & PW_SW_TAIL_OFF)) return;
    const int ns = (int)steps.size();
    for (int si = 0; si + 1 < ns; si++) {
        Step& s = steps[si];
        if (s.kind != S_PW || !s.bx || s.in1 >= 0 || s.in2 >= 0 || s.out < 0 || s.out == v_logits || s.out == v_emb || vals[s.out].external) continue;
        int readers = 0;
        for (int k = 0; k < ns; k++)
            for (int v : {steps[k].in0, steps[k].in1, steps[k].in2}) readers += v == s.out;
        if (readers != 1 || steps[si + 1].in0 != s.out) continue;
        const Step& c = steps[si + 1];
        PwTail t;
        t.H = s.H; t.W = s.W;
        if (c.kind == S_DW && c.sh == 1 && c.sw == 1 && c.kh == c.kw && (c.kh == 3 || c.kh == 5) && c.Ho == c.H && c.Wo == c.W && c.H == s.H && c.W == s.W &&
            c.C == s.Co && c.Co == s.Co && c.pt == (c.kh - 1) / 2 && c.pl == (c.kw - 1) / 2) {
            t.kind = 2; t.k = c.kh; t.pt = c.pt; t.pl = c.pl; t.act = c.act;
        } else if (c.kind == S_MEAN_PARTIAL && si + 2 < ns && steps[si + 2].kind == S_MEAN_FINISH && steps[si + 2].in0 == c.out && c.C == s.Co) {
            t.kind = 1;
        } else continue;
        PwParams p{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, s.H * s.W, s.Co, s.C, s.H * s.W, s.act};
        p.prec = precision; p.sw = pw_sw;
        // (tests: BNHIP_PW_TAIL_FORM=<wm>,<nt> names the form a forced engine plans with - it stands where the tuners do not run)
        int want_wm = 0, want_nt = 6;
        if (const char* e = getenv("BNHIP_PW_TAIL_FORM")) { if (sscanf(e, "%d,%d", &want_wm, &want_nt) != 2) { want_wm = 0; want_nt = 6; } }
        int fit = 0, forced_fit = 0;
        for (int wm : {14, 13, 15}) if (pw_tail_ok(p, t, 6, wm)) { if (!fit) fit = wm; if (wm == want_wm && pw_tail_ok(p, t, want_nt, wm)) forced_fit = wm; }
        if (!fit) continue;
        s.tail = t.kind;
        if (pw_sw & PW_SW_TAIL_FORCE) { s.wm = s.wm_full = forced_fit ? forced_fit : fit; s.nt = s.nt_full = forced_fit ? want_nt : 6; }
    }
}

// ================================================================================================ build
bool Engine::build(TflModel m, int dev, int maxb, bool plan_only, std::string* err, int* code) {
    device = dev;
    max_batch = maxb;
    pw_sw = pw_switches_from_env();      // (tests flip these between engines of one process; nothing reads them after this line)
    if (const char* e = getenv("BNHIP_NORM_RESIDENT")) norm_resident = atoi(e) != 0;
    if (const char* e = getenv("BNHIP_FOLD_PROJ")) fold_proj = atoi(e) != 0;
    const PlanSwitches sw;
    *code = BNHIP_E_UNSUPPORTED;
    // graph rewrites first (float16 constants behind DEQUANTIZE, unfolded batch norm, PAD + VALID convolutions): the
    // patterns below then see one canonical form whatever the exporter emitted
    if (!run_graph_passes(&m, err)) return false;
    if (!select_outputs(m, &logits_output, &embedding_output)) {
        *code = BNHIP_E_INVALID;
        *err = "logits_output / embedding_output do not name two distinct graph outputs";
        return false;
    }
    Lowering L(*this, m, sw);
    if (!L.input_values() || !L.match_frontends() || !L.frontend() || !L.ops() || !L.bind_outputs()) {
        *err = L.err; *code = L.code;
        return false;
    }
    tensor_value = L.tv;
    mark_tails();
    find_norm_pair();
    find_fold_pair();

    mark_liveness(vals, steps);
    if (v_emb >= 0) vals[v_emb].last = (int)steps.size();      // keep until copy-out
    // the kernels index activations with 32-bit element offsets (batch x per-clip elements): refuse a max_batch that a
    // tensor of this model would overflow rather than compute with wrapped addresses
    for (const Value& v : vals)
        if (v.elems * (size_t)max_batch >= ((size_t)1 << 31)) {
            *err = "max_batch too large for this model: a " + std::to_string(v.elems) + "-element activation times " +
                   std::to_string(max_batch) + " clips exceeds 32-bit indexing";
            *code = BNHIP_E_INVALID;
            return false;
        }
    // The plan is laid out twice: for max_batch clips (unsplit calls) and for one lane's share.  Lanes drift apart in
    // time, and values that reuse each other's memory have different per-clip sizes, so addressing lanes as clip offsets
    // into ONE liveness-reused layout lets lane 0's step-k output overwrite lane 1's still-live step-j input: each lane
    // gets its own copy of the (smaller) lane layout instead.
    n_lanes = std::max(1, std::min(n_lanes, kMaxLanes));
    lane_cap = (max_batch + n_lanes - 1) / n_lanes;
    // (a folded projection's operands - its input and gate - are read by the launch of the NEXT step: for the layout they live one
    // step longer, so that step's outputs never land on them; the plan's own liveness, which pick_split reads, is unchanged)
    const int fv0 = fold_pair >= 0 ? steps[fold_pair].in0 : -1, fv1 = fold_pair >= 0 ? steps[fold_pair].in1 : -1;
    const int fl0 = fv0 >= 0 ? vals[fv0].last : 0, fl1 = fv1 >= 0 ? vals[fv1].last : 0;
    if (fv0 >= 0) vals[fv0].last = std::max(fl0, fold_pair + 1);
    if (fv1 >= 0) vals[fv1].last = std::max(fl1, fold_pair + 1);
    act_bytes = plan_arena(vals, steps, (size_t)max_batch, false, no_reuse);
    lane_bytes = n_lanes > 1 ? align_up(plan_arena(vals, steps, (size_t)lane_cap, true, no_reuse), 256) : 0;
    act_bytes = std::max(act_bytes, lane_bytes * (size_t)n_lanes);
    if (fv0 >= 0) vals[fv0].last = fl0;
    if (fv1 >= 0) vals[fv1].last = fl1;
    pick_split();

    w_bytes = L.w.img.size() * sizeof(float);
    if (plan_only) { device = -1; *code = BNHIP_OK; return true; }   // CPU-side planning only (tests, describe)
    return bind_device(L.w, err, code);
}

}  // namespace bnhip
