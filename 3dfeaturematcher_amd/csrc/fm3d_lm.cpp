// fm3d_lm.cpp -- the host side of the LM normals (fm3d_lm2.hip): the launch over one or several
// frame pairs' points (run_lm, run_lm_multi: the pipeline's too) and fm3d_optimize_normals.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fm3d_ctx.h"

using fm3d::LevelDesc;

using namespace fm3d_host;

namespace fm3d_host {  // (declared in fm3d_ctx.h)

void fill_lm_cycles(const fm3d_ctx* c, const unsigned long long* cnt, fm3d_lm_stats* st) {
    st->groups = c->lmGroups;
    st->passes = (int64_t)cnt[3];
    st->cycles_terms = (int64_t)cnt[4];
    st->cycles_chain = (int64_t)cnt[5];
    st->cycles_control = (int64_t)cnt[6];
    st->cycles_total = (int64_t)cnt[7];
    st->wall_ticks_sum = (int64_t)cnt[8];
    st->wall_ticks_max = (int64_t)cnt[9];
    st->wall_clock_khz = c->wallKhz;
    for (int k = 0; k < 4; k++) {
        st->class_passes[k] = (int64_t)cnt[10 + k];
        st->class_cycles[k] = (int64_t)cnt[14 + k];
    }
    st->last_group_start_ticks = (int64_t)(cnt[18] - cnt[20]);
    st->last_group_end_ticks = (int64_t)(cnt[19] - cnt[20]);
    st->cycles_wait = (int64_t)cnt[24];
    st->chain_rounds = (int64_t)cnt[21];
    st->chain_chunks = (int64_t)cnt[22];
    st->queue_empty_ticks = cnt[25] ? (int64_t)(cnt[25] - cnt[20]) : 0;
}

// The LM kernel's camera: the settings' camera with a principal point of -0.0 replaced by +0.0.
// The kernel's isPixelGood compares bit patterns (0 <= u <= xmax as bits(u) <= bits(xmax)), which
// differs from the reference's comparison only for u == -0.0; u = xd*fx + cx (and the image-1
// centre, the same sum) is -0.0 only when cx is -0.0 and xd*fx is -0.0.  With +0.0 that sum is
// +0.0: the reference's test is true for both zeros, and the bilinear sample at a +-0 coordinate is
// the same.  Every other principal point (zero, negative, outside the image) gives the reference's
// bits: a negative u or NaN lies above bits(xmax) as the reference's comparison is false, and the
// fused a2 = r2 + 2x^2 differs only where x*x is subnormal, where u's float sample coordinate
// rounds to the same value (tests/test_gpu_parity.py::test_principal_point_zero_and_negative).
fm3d::Camera lm_camera(const fm3d::Camera& cam) {
    fm3d::Camera k = cam;
    if (k.cx == 0.) k.cx = 0.;  // -0.0 -> +0.0
    if (k.cy == 0.) k.cy = 0.;
    return k;
}

// the LM launch's workgroups for Ptot points (Ptot < 0: as many as the GPU holds): the settings'
// lmWaves, or every CU at the kernel's occupancy, bounded by the points, the slabs' HBM budget and
// their 32-bit offsets
int lm_groups(fm3d_ctx* c, const void* kptr, int slots, long Ptot, long* out) {
    long groups = c->s.lmWaves;
    if (groups <= 0) {
        int cus = 0, perCU = 0;
        HIPCHK(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
        HIPCHK(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, kptr, fm3d::kLM2Threads, 0));
        if (perCU < 1) perCU = 1;
        groups = (long)cus * perCU;
    }
    if (Ptot >= 0) {
        const long needed = (Ptot + slots - 1) / slots;
        if (groups > needed) groups = needed;
    }
    const size_t ents = (size_t)c->nOffPad * slots;
    // per slot and entry: rays (2 doubles) + I1, fvec dI, two Jacobian dI (float) + compact index
    const size_t perGroup = ents * (2 * sizeof(double) + 5 * 4);
    const size_t budget = (size_t)48 << 30;  // HBM budget for the per-slot pixel slabs
    long cap = (long)(budget / perGroup);
    if (cap < 1) cap = 1;
    if (groups > cap) groups = cap;
    // the summed passes address a slab array with a 32-bit byte offset
    const long cap32 = (long)((((size_t)1 << 32) - ((size_t)1 << 20)) / (ents * sizeof(double) * (FM3D_RAY_AOS ? 2 : 1)));
    if (groups > cap32) groups = cap32;
    if (groups < 1) groups = 1;
    *out = groups;
    return FM3D_OK;
}

// Whether image 1's y axis maps closer to image 2's y axis than to its x axis under q's camera-2
// pose: the projections (no distortion) of the mid-depth points on the rays through image 1's
// principal point and through the pixel below it.  The 64 lanes of an LM chunk are 64 consecutive
// rows of one image-1 column (ensure_offsets: x outer, y inner), so their image-2 samples then run
// down a column and the column-major level copy serves them from 1-3 cache lines (DESIGN.md §3.4,
// "Gather geometry"); a pair rolled by about 90 degrees keeps the rows.
bool lm_prefers_cols(const fm3d_ctx* q) {
    const fm3d::Camera& k = q->cam;
    const double z = 0.5 * (q->s.zThresholdMin + q->s.zThresholdMax);
    const double X[2][3] = {{0., 0., z}, {0., z / k.fy, z}};
    double u[2], v[2];
    for (int i = 0; i < 2; i++) {
        const double* R = q->R2;
        const double x = R[0] * X[i][0] + R[1] * X[i][1] + R[2] * X[i][2] + q->t2[0];
        const double y = R[3] * X[i][0] + R[4] * X[i][1] + R[5] * X[i][2] + q->t2[1];
        const double w = R[6] * X[i][0] + R[7] * X[i][1] + R[8] * X[i][2] + q->t2[2];
        if (!(w > 0.)) return false;
        u[i] = k.fx * x / w;
        v[i] = k.fy * y / w;
    }
    return std::fabs(v[1] - v[0]) > std::fabs(u[1] - u[0]);  // false for NaN
}

// LM normals over the points of nProb frame pairs in ONE launch on c's stream (c's slabs, queue
// and launch counters): the slots that find one pair's points used up take the next pair's, so
// a second pair fills the launch's end-of-queue tail (fm3d_pipeline_link).  Every problem's
// context must be ordered before this stream by the caller (its points, pyramids).
int run_lm_multi(fm3d_ctx* c, const LMSrc* src, int nProb, fm3d_lm_stats* stats, hipEvent_t e0, hipEvent_t e1) {
    int r;
    if (nProb < 1 || nProb > fm3d::kLMMaxProblems) return fail(c, FM3D_ERR_INVALID, "bad LM problem count");
    if ((r = ensure_offsets(c))) return r;
    const fm3d::Camera cam = lm_camera(c->cam);
    const int levels = c->s.pyramids;
    long Ptot = 0;
    for (int j = 0; j < nProb; j++) {
        fm3d_ctx* q = src[j].c;
        if (q->pyr1.empty()) return fail(c, FM3D_ERR_INVALID, "fm3d_set_images (NormalOptimizer::setImages) not called");
        if (!q->haveG12) return fail(c, FM3D_ERR_INVALID, "g12 not set (SingleCameraTriangulator::setg12)");
        if (q != c && (q->device != c->device || q->s.pyramids != levels || q->s.pixelsRay != c->s.pixelsRay ||
                       std::memcmp(&q->cam, &c->cam, sizeof(c->cam)) != 0 || q->s.boundWidth != c->s.boundWidth ||
                       q->s.boundHeight != c->s.boundHeight || q->s.zThresholdMax != c->s.zThresholdMax ||
                       q->s.epsilonLMMIN != c->s.epsilonLMMIN || q->s.lmReduction != c->s.lmReduction))
            return fail(c, FM3D_ERR_INVALID, "linked contexts need one device, camera and LM settings");
        const int P = src[j].P;
        HIPCHK(c, q->lmNormals.ensure((size_t)(P + 1) * 3 * sizeof(double)));
        HIPCHK(c, q->lmStatus.ensure((size_t)(P + 1) * sizeof(int)));
        HIPCHK(c, q->lmInfo.ensure((size_t)(P + 1) * 8 * sizeof(int)));
        HIPCHK(c, q->lmNfev.ensure((size_t)(P + 1) * 8 * sizeof(int)));
        HIPCHK(c, q->lmMdat.ensure((size_t)(P + 1) * sizeof(int)));
        HIPCHK(c, q->pcnt.ensure(64));
        Ptot += P;
    }
    HIPCHK(c, c->lmQueue.ensure(64 * sizeof(int)));
    HIPCHK(c, c->lmStat.ensure(256));
    // persistent workgroups of fm3d::kLM2Slots term waves (one point each) + a chain wave, or in the
    // tree-reduction mode kLM2Slots + 1 term waves; slots refill from the queue (fm3d_lm2.hip)
    // the settings field alone picks the mode (no environment override: ADVICE r05; the tree mode
    // fails the parity gate, profiles/r05_full_parity.json)
    if (c->s.lmReduction != 0 && c->s.lmReduction != 1)
        return fail(c, FM3D_ERR_INVALID, "lmReduction must be 0 (pixel order) or 1 (tree)");
    const bool tree = c->s.lmReduction != 0;
    const int slots = fm3d::kLM2Slots + (tree ? 1 : 0);
    // one pose for all problems: the single-pose kernel (entry 0 of the table serves them all)
    bool multiPose = false;
    for (int j = 1; j < nProb; j++)
        multiPose |= std::memcmp(src[j].c->R2, src[0].c->R2, sizeof(c->R2)) != 0 ||
                     std::memcmp(src[j].c->t2, src[0].c->t2, sizeof(c->t2)) != 0;
    // image 2's layout for the gathers: the columns only if every pair's pose chooses them.
    // FM3D_LM_IMG2 = rows | cols | auto (default) forces one: the results are the same bits (tests, A/B)
    bool cols = true;
    for (int j = 0; j < nProb; j++) cols &= lm_prefers_cols(src[j].c);
    if (const char* lay = getenv("FM3D_LM_IMG2")) {
        if (!std::strcmp(lay, "rows")) cols = false;
        else if (!std::strcmp(lay, "cols")) cols = true;
        else if (std::strcmp(lay, "auto")) return fail(c, FM3D_ERR_INVALID, "FM3D_LM_IMG2 must be rows, cols or auto");
    }
    for (int j = 0; j < nProb; j++) src[j].c->lmCols = cols;
    c->lmCols = cols;
    const void* const kptrs[2][2][2] = {
        {{reinterpret_cast<const void*>(fm3d::lm2_kernel<false, false, false>),
          reinterpret_cast<const void*>(fm3d::lm2_kernel<false, false, true>)},
         {reinterpret_cast<const void*>(fm3d::lm2_kernel<true, false, false>),
          reinterpret_cast<const void*>(fm3d::lm2_kernel<true, false, true>)}},
        {{reinterpret_cast<const void*>(fm3d::lm2_kernel<false, true, false>),
          reinterpret_cast<const void*>(fm3d::lm2_kernel<false, true, true>)},
         {reinterpret_cast<const void*>(fm3d::lm2_kernel<true, true, false>),
          reinterpret_cast<const void*>(fm3d::lm2_kernel<true, true, true>)}}};
    const void* kptr = kptrs[tree][multiPose][cols];  // [TREE][MULTI][COLS]
    long groups = 0;
    int r0;
    if ((r0 = lm_groups(c, kptr, slots, Ptot, &groups))) return r0;
    const size_t ents = (size_t)c->nOffPad * slots;
    // +8 KiB: the passes prefetch up to eight 64-entry chunks past a slot's last entry
    HIPCHK(c, c->slab.ensure(ents * 2 * sizeof(double) * groups + 16384));
    HIPCHK(c, c->slabI1.ensure(ents * 5 * 4 * groups + 16384));
    fm3d::LMParams p{};
    p.nProb = nProb;
    p.cam = cam;
    {   // per problem: its pose as a small global table (re-read per chunk by the LM kernel), and
        // the problem table; both from pinned memory (the copies may run after this returns)
        HIPCHK(c, hipEventSynchronize(c->evProj));  // the previous launch's copies out of hProj ran
        const size_t pcBytes = (sizeof(fm3d::ProjConst) + 255) / 256 * 256;
        HIPCHK(c, c->hProj.ensure(pcBytes * nProb + sizeof(fm3d::LMProblem) * nProb));
        char* hp = c->hProj.as<char>();
        fm3d::LMProblem* hpr = (fm3d::LMProblem*)(hp + pcBytes * nProb);
        HIPCHK(c, c->lmProj.ensure(pcBytes * nProb + sizeof(fm3d::LMProblem) * nProb));
        const size_t Gn = (size_t)groups * slots * c->nOffPad;  // entries per slab array
        for (int j = 0; j < nProb; j++) {
            fm3d_ctx* q = src[j].c;
            fm3d::ProjConst& pc = *(fm3d::ProjConst*)(hp + pcBytes * j);
            std::memcpy(pc.R, q->R2, sizeof(pc.R));
            std::memcpy(pc.t, q->t2, sizeof(pc.t));
            pc.cam = cam;
            pc.k2d = 2. * cam.k[2];
            pc.k3d = 2. * cam.k[3];
            pc.slabRX = (const char*)c->slab.p;
            pc.slabRY = FM3D_RAY_AOS ? pc.slabRX + sizeof(double) : pc.slabRX + Gn * sizeof(double);
            pc.slabI1 = (const char*)c->slabI1.p;
            pc.slabDF = (char*)c->slabI1.p + Gn * 4;
            pc.slabDJ0 = pc.slabDF + Gn * 4;
            pc.slabDJ1 = pc.slabDJ0 + Gn * 4;
            fm3d::LMProblem& pr = hpr[j];
            pr.points = q->pts.as<double>();
            pr.Pdev = src[j].Pdev;
            pr.P = src[j].P;
            pr.lvl = q->lvlDesc.as<LevelDesc>();
            pr.normals = q->lmNormals.as<double>();
            pr.status = q->lmStatus.as<int>();
            pr.info = q->lmInfo.as<int>();
            pr.nfev = q->lmNfev.as<int>();
            pr.mdat = q->lmMdat.as<int>();
            pr.stat = (unsigned long long*)(q->pcnt.as<char>() + 16);
            pr.projOff = (unsigned)(pcBytes * j);
        }
        HIPCHK(c, hipMemcpyAsync(c->lmProj.p, hp, pcBytes * nProb + sizeof(fm3d::LMProblem) * nProb,
                                 hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipEventRecord(c->evProj, c->stream));
        p.proj = c->lmProj.as<fm3d::ProjConst>();
        p.prob = (const fm3d::LMProblem*)(c->lmProj.as<char>() + pcBytes * nProb);
    }
    p.levels = levels;
    p.offsets = c->offsets.as<int2>();
    p.nOff = c->nOff;
    p.nOffPad = c->nOffPad;
    p.boundW = c->s.boundWidth;
    p.boundH = c->s.boundHeight;
    p.epsfcn = c->s.epsilonLMMIN;
    p.cmax = (int)(2 * c->s.zThresholdMax);  // isInBoundingBox: int cMax = 2*z_threshold_max_ (:648)
    p.queue = c->lmQueue.as<int>();
    p.slab = c->slab.as<double>();
    p.slabI1 = c->slabI1.as<float>();
    p.nWaves = groups;
    p.statEval = c->lmStat.as<unsigned long long>();
    p.statPix = c->lmStat.as<unsigned long long>() + 1;
    p.overflow = (int*)(c->lmStat.as<unsigned long long>() + 2);
    p.statPass = c->lmStat.as<unsigned long long>() + 3;
    c->lmGroups = groups;
    {   // guards against a broken state machine (never expected to trigger): passes per slot
        // <= its points x levels x (300 evaluations + QR passes), and a wall-clock limit
        const long long perSlot = (Ptot + groups * slots - 1) / (groups * slots) + 1;
        p.maxIter = perSlot * (long long)(levels + 1) * 1600 + 10000;
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device) != hipSuccess || khz <= 0) khz = 100000;
        const char* ms = getenv("FM3D_LM_MAX_SECONDS");  // watchdog (tests lower it; fractions allowed)
        const double secs = ms && atof(ms) > 0 ? atof(ms) : 300.;
        p.maxTicks = (long long)((double)khz * 1000. * secs);
        c->wallKhz = khz;
        const char* co = getenv("FM3D_LM_COOP");  // A/B switch for the tail help
        p.coop = co ? atoi(co) : 1;
        if (tree) p.coop = 0;  // a helper's chunks would leave the lanes' chunk order of the tree
        const char* sf = getenv("FM3D_LM_SAFE");  // test switch: the guarded pass forms only
        p.safe = sf ? atoi(sf) : 0;
    }
    // the counters (incl. the overflow word) are reset for every call, also for P == 0; with points,
    // the queue, the min-start word and every problem's statuses / info / nfev too -- one kernel
    {
        fm3d::LMReset rz{};
        rz.stat = c->lmStat.as<unsigned long long>();
        rz.queue = Ptot > 0 ? c->lmQueue.as<int>() : nullptr;
        rz.nProb = nProb;
        for (int j = 0; j < nProb; j++) {
            fm3d_ctx* q = src[j].c;
            rz.pcnt16[j] = q->pcnt.as<int>() + 4;
            rz.status[j] = q->lmStatus.as<int>();
            rz.info[j] = q->lmInfo.as<int>();
            rz.nfev[j] = q->lmNfev.as<int>();
            rz.P[j] = Ptot > 0 && src[j].P > 0 ? src[j].P : 0;
        }
        if (Ptot > 0) HIPCHK(c, hipEventRecord(e0, c->stream));
        fm3d::launch_lm_reset(rz, c->stream);
        HIPCHK(c, hipGetLastError());
    }
    if (Ptot > 0) {
        // one launch: every slot runs its point through all levels, coarsest first
        // (optimize_pyramid :225-241)
        // through the runtime's launch by address (not a call through a cast function pointer, which
        // the host sanitizers' function-type check rejects: tests/test_sanitizers.py)
        void* kargs[] = {&p};
        HIPCHK(c, hipLaunchKernel(kptr, dim3((unsigned)groups), dim3(fm3d::kLM2Threads), kargs, 0, c->stream));
        HIPCHK(c, hipEventRecord(e1, c->stream));
    }
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->points_in = Ptot;
    }
    return FM3D_OK;
}

// LM normals over c's own points (c->pts: P, or the bound P with the count at Pdev)
int run_lm(fm3d_ctx* c, int P, const int* Pdev, fm3d_lm_stats* stats, hipEvent_t e0, hipEvent_t e1) {
    const LMSrc one{c, P, Pdev};
    return run_lm_multi(c, &one, 1, stats, e0, e1);
}

}  // namespace fm3d_host

extern "C" {

int fm3d_optimize_normals(fm3d_ctx* c, double* points, int P, double* normals, int32_t* status, int32_t* info,
                          int32_t* nfev, int* nKept, fm3d_lm_stats* stats) {
    if (!c || !nKept || P < 0 || (P && (!points || !normals))) return fail(c, FM3D_ERR_INVALID, "bad argument");
    hipSetDevice(c->device);
    int r;
    if ((r = upload(c, c->pts, points, (size_t)P * 3 * sizeof(double)))) return r;
    if ((r = run_lm(c, P, nullptr, stats, c->ev[EV_LM_START], c->ev[EV_END]))) return r;
    std::vector<double> nrm((size_t)P * 3);
    std::vector<int> st(P), inf((size_t)P * 8), nf((size_t)P * 8);
    unsigned long long cnt[26] = {};
    if (P) {
        HIPCHK(c, hipMemcpyAsync(nrm.data(), c->lmNormals.p, nrm.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(st.data(), c->lmStatus.p, st.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(inf.data(), c->lmInfo.p, inf.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(nf.data(), c->lmNfev.p, nf.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(cnt, c->lmStat.p, sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int overflow = 0;  // lmStat is reset by run_lm for every call (P == 0 included)
    HIPCHK(c, hipMemcpy(&overflow, c->lmStat.as<unsigned long long>() + 2, sizeof(int), hipMemcpyDeviceToHost));
    if (overflow) return fail(c, FM3D_ERR_HIP, "LM kernel iteration guard tripped (internal error)");
    float ms = 0.f;
    if (P) hipEventElapsedTime(&ms, c->ev[EV_LM_START], c->ev[EV_END]);
    // erase semantics (normaloptimizer.cpp:366,378): stable compaction, input order kept
    int kept = 0;
    bool nanPlane = false;
    for (int i = 0; i < P; i++) {
        if (status) status[i] = st[i];
        if (info) std::memcpy(&info[(size_t)8 * i], &inf[(size_t)8 * i], 8 * sizeof(int));
        if (nfev) std::memcpy(&nfev[(size_t)8 * i], &nf[(size_t)8 * i], 8 * sizeof(int));
        if (st[i] == FM3D_ST_NAN_PLANE) nanPlane = true;
        if (st[i] == FM3D_ST_OK) {
            for (int k = 0; k < 3; k++) {
                points[3 * kept + k] = points[3 * i + k];
                normals[3 * kept + k] = nrm[3 * i + k];
            }
            kept++;
        }
    }
    *nKept = kept;
    if (stats) {
        stats->points_in = P;
        stats->points_kept = kept;
        stats->evaluations = (int64_t)cnt[0];
        stats->pixel_evaluations = (int64_t)cnt[1];
        for (int i = 0; i < P; i++)
            if (st[i] >= 0 && st[i] < 8) stats->drops[st[i]]++;
        stats->kernel_ms = ms;
        fill_lm_cycles(c, cnt, stats);
    }
    if (nanPlane && c->s.strictNanExit)
        return fail(c, FM3D_ERR_NAN_PLANE, "projectPointToPlane hit NaN (reference: exit(-6))");
    return FM3D_OK;
}

}  // extern "C"
