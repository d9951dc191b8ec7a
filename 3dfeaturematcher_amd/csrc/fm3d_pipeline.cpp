// fm3d_pipeline.cpp -- the staged pipeline: one frame pair's inputs resident in HBM and the whole
// path, its front half alone, the verified forms (synchronous, and as submit / wait) or the NCC scoring
// queued on the context stream (fm3d_pipeline_*), and the multi-GPU host's entry points
// (fm3d_internal_*, fm3d_internal.h).  What is queued and not yet waited for is c->pipe.state
// (fm3d_ctx.h PairState): see require().
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fm3d_ctx.h"
#include "fm3d_internal.h"

using namespace fm3d_host;

namespace {

// The state rule of an entry point, first thing: the code and message of the first condition that
// fails (the messages are API: DESIGN.md §2.1, tests/test_gpu_pipeline_states.py).
int require(fm3d_ctx* c, Need need) {
    if (need == Need::StagedIdle && (!c || !c->staged)) return fail(c, FM3D_ERR_INVALID, "fm3d_pipeline_upload not called");
    if (!c) return FM3D_ERR_INVALID;
    const PairState s = c->pipe.state;
    // a verified pair has waits of its own, and they serve nothing else
    if (need != Need::StagedIdle && need != Need::Idle) {
        if (s == PairState::Verified && need != Need::Verified)
            return fail(c, FM3D_ERR_INVALID, "a verified frame pair is pending: fm3d_pipeline_wait_verified");
        if (s == PairState::DltVerified && need != Need::DltVerified)
            return fail(c, FM3D_ERR_INVALID, "a verified front half is pending: fm3d_pipeline_wait_dlt_verified");
    }
    if (need == Need::Verified && s != PairState::Verified)
        return fail(c, FM3D_ERR_INVALID, "no verified frame pair submitted (fm3d_pipeline_submit_verified)");
    if (need == Need::DltVerified && s != PairState::DltVerified)
        return fail(c, FM3D_ERR_INVALID, "no verified front half submitted (fm3d_pipeline_submit_dlt_verified)");
    if ((need == Need::StagedIdle || need == Need::Idle) && s != PairState::Idle)
        return fail(c, FM3D_ERR_INVALID, "a submitted frame pair is pending: fm3d_pipeline_wait first");
    if (need == Need::Full) {
        if (s == PairState::Idle) return fail(c, FM3D_ERR_INVALID, "no frame pair submitted (fm3d_pipeline_submit)");
        if (s == PairState::DltFront) return fail(c, FM3D_ERR_INVALID, "a front half is pending: fm3d_pipeline_wait_dlt");
        if (s == PairState::Ncc) return fail(c, FM3D_ERR_INVALID, "an NCC scoring is pending: fm3d_pipeline_wait_ncc");
    }
    if (need == Need::Dlt && s != PairState::DltFront)
        return fail(c, FM3D_ERR_INVALID, "no front half submitted (fm3d_pipeline_submit_dlt)");
    if (need == Need::Ncc && s != PairState::Ncc)
        return fail(c, FM3D_ERR_INVALID, "no NCC scoring submitted (fm3d_pipeline_submit_ncc)");
    return FM3D_OK;
}

// one frame pair's host inputs, as the ABI's submit / upload calls take them
struct PairInputs {
    const void* descA;
    int nA;
    const void* descB;
    int nB, dim, type;
    const fm3d_point2f *kpts1, *kpts2;
    const uint8_t *img1, *img2;  // both null: no images staged (C2's match + DLT needs none)
    int width, height, queryOffset;
};

// the head every path's fm3d_pipeline_stats share: zeroed, the staged sizes, the counts and, when a
// front half ran to its end (timed) and recorded its stage events, match_ms (row constants, knn, NNDR
// and its compaction: one stage since NNDR is fused into the match's last launch; nndr_ms stays 0) and
// triangulate_ms
void stats_head(fm3d_ctx* c, int K, int P, bool timed, fm3d_pipeline_stats* stats) {
    std::memset(stats, 0, sizeof(*stats));
    stats->queries = c->pipe.nA;
    stats->trains = c->pipe.nB;
    stats->matches = K;
    stats->inliers = P;
    if (!timed || !c->pipe.stageEv) return;
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev[EV_FRONT_START], c->ev[EV_MATCH_DONE]);
    stats->match_ms = ms;
    hipEventElapsedTime(&ms, c->ev[EV_MATCH_DONE], c->ev[EV_DLT_DONE]);
    stats->triangulate_ms = ms;
}

// the inputs of one frame pair into HBM on the context stream (pinned staging, asynchronous):
// descriptors, keypoints, both images and their pyramids (a6, normaloptimizer.cpp:206-221)
int stage_pipeline(fm3d_ctx* c, const PairInputs& in, bool speculate = false) {
    if (!in.kpts1 || !in.kpts2) return fail(c, FM3D_ERR_INVALID, "null argument");
    const int nA = in.nA, nB = in.nB;
    int t, dp, r;
    // the previous pair's copies out of the staging buffers have run: one wait, then every H2D of
    // this pair is queued without another (the call returns before they execute)
    if ((r = staging_wait(c))) return r;
    if ((r = stage_descriptors(c, in.descA, nA, in.descB, nB, in.dim, in.type, &t, &dp, false, speculate))) return r;
    if ((r = upload_pinned(c, c->kp1, c->hK1, in.kpts1, (size_t)nA * sizeof(fm3d_point2f)))) return r;
    if ((r = upload_pinned(c, c->kp2, c->hK2, in.kpts2, (size_t)nB * sizeof(fm3d_point2f)))) return r;
    if (in.img1 || in.img2) {  // records evStage
        if ((r = set_images_impl(c, in.img1, in.img2, in.width, in.height, in.width, false, false))) return r;
    } else {  // no images (C2's match + DLT needs none): the context keeps the ones it has, if any
        HIPCHK(c, hipEventRecord(c->evStage, c->stream));
    }
    if (!c->haveG12) {
        double g[16];
        if ((r = fm3d_setg12(c, c->s.pos1, c->s.pos2, c->s.pos1 + 3, c->s.pos2 + 3, g))) return r;
    }
    if ((r = ensure_offsets(c))) return r;
    c->pipe.nA = nA;
    c->pipe.nB = nB;
    c->pipe.dim = in.dim;
    c->pipe.type = t;
    c->pipe.dimPad = dp;
    c->pipe.queryOffset = in.queryOffset;
    c->staged = true;
    c->gateStaged = false;
    return FM3D_OK;
}

// The front half on the staged inputs (EV_FRONT_START .. EV_DLT_DONE) is match -> NNDR -> compaction
// (front_match), then DLT triangulation -> compaction (front_dlt), sized by the query count: the match
// count K and the inlier count P stay on the device (c->pcnt[0], [1]) and bound nothing the host launches,
// so the stages queue without a host round trip (c->matches, c->pts, c->srcIdx hold K / P entries)
int front_match(fm3d_ctx* c) {
    const int nA = c->pipe.nA, nB = c->pipe.nB;
    int r;
    HIPCHK(c, c->pcnt.ensure(64));
    int* cnt = c->pcnt.as<int>();
    // Fm3d.guidedMatchPx: the epipolar gate over the staged keypoints (kp1 holds this share's queries),
    // its lines and (u, v) computed once per upload and pose
    fm3d::EpiGate gate{};
    const bool guided = c->s.guidedMatchPx > 0.;
    if (guided) {
        if (!c->gateStaged) {
            if ((r = make_gate(c, c->kp1.as<fm3d_point2f>(), nA, c->kp2.as<fm3d_point2f>(), nB, c->s.guidedMatchPx, &gate)))
                return r;
            c->gateStaged = true;
        }
        gate.lines = c->gLines.as<float4>();
        gate.uv = c->gUV.as<float2>();
        gate.tau = c->s.guidedMatchPx * 2.0 / (c->cam.fx + c->cam.fy);
    }
    HIPCHK(c, hipEventRecord(c->ev[EV_FRONT_START], c->stream));
    // a1: match + NNDR (+ the stable compaction of the kept matches, fused into the NNDR launch)
    if ((r = ensure_scan_tmp(c, nA))) return r;
    HIPCHK(c, c->matches.ensure((size_t)(nA + 1) * sizeof(fm3d_dmatch)));
    MatchOpts o;
    o.eps = c->s.nndrEpsilon;
    o.queryOffset = c->pipe.queryOffset;
    o.compactOut = c->matches.as<fm3d_dmatch>();
    o.compactCount = cnt + 0;
    o.gate = guided ? &gate : nullptr;
    o.crossCheck = c->s.crossCheck;
    if ((r = run_match(c, nA, nB, c->pipe.type, c->pipe.dimPad, o))) return r;
    // the stage boundaries (EV_MATCH_DONE, EV_DLT_DONE) only when asked for: a timed event between
    // two launches costs the C2 step 4-10 us of gap (rocprofv3 trace, round 5); FM3D_STAGE_EVENTS=0
    // leaves only the step's own EV_FRONT_START / EV_END
    c->pipe.stageEv = env_on("FM3D_STAGE_EVENTS");
    if (c->pipe.stageEv) HIPCHK(c, hipEventRecord(c->ev[EV_MATCH_DONE], c->stream));
    return FM3D_OK;
}

// hostCnt: the DLT kernel also stores (K, P) there (a device pointer to page-locked memory)
int front_dlt(fm3d_ctx* c, int* hostCnt) {
    const int nA = c->pipe.nA;
    int r;
    int* cnt = c->pcnt.as<int>();
    // a4, a5: triangulate (matches are device resident; K <= nA)
    HIPCHK(c, c->triPts.ensure((size_t)(nA + 1) * 3 * sizeof(double)));
    HIPCHK(c, c->triMask.ensure((size_t)(nA + 1) * sizeof(int)));
    HIPCHK(c, c->pts.ensure((size_t)(nA + 1) * 3 * sizeof(double)));
    HIPCHK(c, c->srcIdx.ensure((size_t)(nA + 1) * sizeof(int)));
    fm3d::TriParams tp = tri_params(c, nA, c->pipe.queryOffset);
    tp.Kdev = cnt + 0;
    fm3d::LookBack lb;  // DLT with the inliers' compaction fused (launch_triangulate_compact)
    if ((r = make_lookback(c, fm3d::triangulate_compact_blocks(nA), &lb))) return r;
    fm3d::launch_triangulate_compact(tp, c->pts.as<double>(), c->srcIdx.as<int>(), cnt + 1, lb, c->stream, hostCnt);
    HIPCHK(c, hipGetLastError());
    if (c->pipe.stageEv) HIPCHK(c, hipEventRecord(c->ev[EV_DLT_DONE], c->stream));
    return FM3D_OK;
}

int pipeline_front(fm3d_ctx* c, int* hostCnt = nullptr) {
    if (int r = front_match(c)) return r;
    return front_dlt(c, hostCnt);
}

// front_dlt with the counts written to page-locked memory (c->hSmall) by the DLT kernel itself (no
// copy launch), after the match half when withMatch; then the end event
int front_with_counts(fm3d_ctx* c, bool withMatch) {
    int r;
    HIPCHK(c, c->hSmall.ensure(sizeof(PipeSmall)));
    void* dcnt = nullptr;
    HIPCHK(c, hipHostGetDevicePointer(&dcnt, c->hSmall.as<PipeSmall>()->cnt, 0));
    if ((r = withMatch ? pipeline_front(c, (int*)dcnt) : front_dlt(c, (int*)dcnt))) return r;
    HIPCHK(c, hipEventRecord(c->ev[EV_END], c->stream));
    return FM3D_OK;
}

// the survivor records of c's pair (after its LM normals, in stream order), then one D2H of the
// counts, the pair's LM counters and the LM launch's counters (lmStat: the launching context's)
int enqueue_epilogue(fm3d_ctx* c, fm3d_record* out, const void* lmStat) {
    const int nA = c->pipe.nA;
    int* cnt = c->pcnt.as<int>();
    HIPCHK(c, c->recTmp.ensure((size_t)(nA + 1) * sizeof(fm3d_record)));
    HIPCHK(c, c->recFlag.ensure((size_t)(nA + 1) * sizeof(int)));
    if (!out) {
        HIPCHK(c, c->records.ensure((size_t)(nA + 1) * sizeof(fm3d_record)));
        out = c->records.as<fm3d_record>();
    }
    c->pipe.pendOut = out;
    fm3d::launch_make_records(c->matches.as<fm3d_dmatch>(), c->srcIdx.as<int>(), nA, cnt + 1, c->pts.as<double>(),
                              c->lmNormals.as<double>(), c->lmStatus.as<int>(), c->recTmp.as<fm3d_record>(),
                              c->recFlag.as<int>(), c->stream);
    fm3d::launch_compact_records(c->recTmp.as<fm3d_record>(), c->recFlag.as<int>(), nA, cnt + 1, out, cnt + 2,
                                 c->scanTmp.p, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, c->hSmall.ensure(sizeof(PipeSmall)));
    PipeSmall* hs = c->hSmall.as<PipeSmall>();
    HIPCHK(c, hipMemcpyAsync(hs->cnt, cnt, sizeof(hs->cnt) + sizeof(hs->prob), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hs->lm, lmStat, sizeof(hs->lm), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(c->ev[EV_END], c->stream));
    return FM3D_OK;
}

// the LM normals over the front half's inliers, then the records and the small D2H
int enqueue_normals(fm3d_ctx* c, fm3d_record* out, fm3d_lm_stats* ls) {
    if (int r = run_lm(c, c->pipe.nA, c->pcnt.as<int>() + 1, ls, c->ev[EV_NORMAL_START], c->ev[EV_NORMAL_END])) return r;
    return enqueue_epilogue(c, out, c->lmStat.p);
}

// the whole path on the staged inputs, queued on the context stream: front half, LM normals over
// the device-counted inliers (a6-a15; the pyramids were built at staging: images are inputs of the
// path), survivor records (compacted into out, or the internal buffer), then one D2H of the counts
// and the LM counters into pinned memory.  Nothing here waits for the device.
int enqueue_full(fm3d_ctx* c, fm3d_record* out, fm3d_lm_stats* ls) {
    if (int r = pipeline_front(c)) return r;
    return enqueue_normals(c, out, ls);
}

// the leader's pair with its members' queued front halves: ONE LM launch over all these pairs'
// points on the leader's stream (after every member's front half), then each pair's records on
// its own stream
int enqueue_linked(fm3d_ctx* c, const std::vector<fm3d_ctx*>& ms, fm3d_lm_stats* ls) {
    int r;
    if ((r = pipeline_front(c))) return r;
    std::vector<LMSrc> src;
    for (fm3d_ctx* m : ms) {
        HIPCHK(c, hipStreamWaitEvent(c->stream, m->pipe.evFront, 0));
        src.push_back({m, m->pipe.nA, m->pcnt.as<int>() + 1});
        HIPCHK(c, hipEventRecord(m->ev[EV_NORMAL_START], c->stream));
    }
    src.push_back({c, c->pipe.nA, c->pcnt.as<int>() + 1});
    if ((r = run_lm_multi(c, src.data(), (int)src.size(), ls, c->ev[EV_NORMAL_START], c->ev[EV_NORMAL_END]))) return r;
    // each member gets its own copy of the launch's counters (on this stream, before evLm): the
    // leader's next run_lm_multi resets c->lmStat, possibly before a member's epilogue has read it
    for (fm3d_ctx* m : ms) {
        HIPCHK(m, m->lmStat.ensure(256));
        HIPCHK(c, hipMemcpyAsync(m->lmStat.p, c->lmStat.p, sizeof(PipeSmall::lm), hipMemcpyDeviceToDevice, c->stream));
    }
    HIPCHK(c, hipEventRecord(c->pipe.evLm, c->stream));
    if ((r = enqueue_epilogue(c, c->pipe.subOut, c->lmStat.p))) return r;
    for (fm3d_ctx* m : ms) {
        HIPCHK(c, hipEventRecord(m->ev[EV_NORMAL_END], c->stream));
        m->pipe.subLm = *ls;
        m->lmGroups = c->lmGroups;
        m->wallKhz = c->wallKhz;
        hipSetDevice(m->device);
        HIPCHK(m, hipStreamWaitEvent(m->stream, c->pipe.evLm, 0));
        if ((r = enqueue_epilogue(m, m->pipe.subOut, m->lmStat.p))) return r;
        m->pipe.state = PairState::Full;
    }
    return FM3D_OK;
}

// after the stream ran enqueue_full: guards, counts and stats (t0: the event the total starts at)
int finalize_full(fm3d_ctx* c, const fm3d_lm_stats& ls, hipEvent_t t0, bool staged_in_step, int* nKept,
                  fm3d_pipeline_stats* stats) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const PipeSmall* hs = c->hSmall.as<PipeSmall>();
    const int K = hs->cnt[0], P = hs->cnt[1], kept = hs->cnt[2];
    c->pipe.K = K;
    c->pipe.P = P;
    // the LM watchdog (maxIter / FM3D_LM_MAX_SECONDS) leaves points in kLMRunning: an error, not drops
    if (hs->lm[2]) return fail(c, FM3D_ERR_HIP, "LM kernel iteration guard tripped (internal error)");
    if (c->s.strictNanExit && P > 0) {  // reference exit(-6) on a NaN plane hit (:465-469)
        std::vector<int> st(P);
        HIPCHK(c, hipMemcpy(st.data(), c->lmStatus.p, (size_t)P * sizeof(int), hipMemcpyDeviceToHost));
        for (int i = 0; i < P; i++)
            if (st[i] == FM3D_ST_NAN_PLANE)
                return fail(c, FM3D_ERR_NAN_PLANE, "projectPointToPlane hit NaN (reference: exit(-6))");
    }
    if (nKept) *nKept = kept;
    if (stats) {
        stats_head(c, K, P, true, stats);
        stats->kept = kept;
        float ms = 0;
        if (staged_in_step) hipEventElapsedTime(&ms, c->ev[EV_SUBMIT_START], c->ev[EV_FRONT_START]);
        stats->pyramid_ms = ms;  // the inputs' H2D + pyramids (fm3d_pipeline_submit only)
        ms = 0;
        hipEventElapsedTime(&ms, c->ev[EV_NORMAL_START], c->ev[EV_NORMAL_END]);
        stats->lm_ms = ms;
        hipEventElapsedTime(&ms, t0, c->ev[EV_END]);
        stats->total_ms = ms;
        stats->lm = ls;
        stats->lm.points_in = P;
        stats->lm.points_kept = kept;
        stats->lm.evaluations = (int64_t)hs->prob[0];  // this pair's (a launch may hold two)
        stats->lm.pixel_evaluations = (int64_t)hs->prob[1];
        stats->lm.kernel_ms = stats->lm_ms;
        fill_lm_cycles(c, hs->lm, &stats->lm);
    }
    return FM3D_OK;
}

// one frame pair staged and queued on c's stream (records into out: device, or null = internal);
// a link member queues its front half only, a leader joins its queued members' pairs
int submit_impl(fm3d_ctx* c, const PairInputs& in, fm3d_record* out) {
    int r;
    if ((r = require(c, Need::Idle))) return r;
    hipSetDevice(c->device);
    HIPCHK(c, hipEventRecord(c->ev[EV_SUBMIT_START], c->stream));
    if ((r = stage_pipeline(c, in))) return r;
    c->pipe.subLm = fm3d_lm_stats{};
    c->pipe.subOut = out;
    if (c->pipe.linkLeader) {  // member: the front half now, the LM with the leader's next pair
        if ((r = pipeline_front(c))) return r;
        HIPCHK(c, hipEventRecord(c->pipe.evFront, c->stream));
        c->pipe.state = PairState::MemberFront;
        return FM3D_OK;
    } else if (!c->pipe.linkMembers.empty()) {
        std::vector<fm3d_ctx*> ms;  // the members with a pair queued since this leader's last launch
        for (fm3d_ctx* m : c->pipe.linkMembers)
            if (m->pipe.state == PairState::MemberFront) ms.push_back(m);
        if ((r = ms.empty() ? enqueue_full(c, out, &c->pipe.subLm) : enqueue_linked(c, ms, &c->pipe.subLm))) return r;
    } else {
        if ((r = enqueue_full(c, out, &c->pipe.subLm))) return r;
    }
    c->pipe.state = PairState::Full;
    return FM3D_OK;
}

// a member whose leader took no pair since its submit: its LM alone, on its own stream
int flush_member(fm3d_ctx* c) {
    if (c->pipe.state != PairState::MemberFront) return FM3D_OK;
    hipSetDevice(c->device);
    if (int r = enqueue_normals(c, c->pipe.subOut, &c->pipe.subLm)) return r;
    c->pipe.state = PairState::Full;
    return FM3D_OK;
}

// after EV_END of front_with_counts: the counts it left in page-locked memory, and the stage times
void report_front_counts(fm3d_ctx* c, int* nInliers, fm3d_pipeline_stats* stats) {
    const PipeSmall* hs = c->hSmall.as<PipeSmall>();
    const int K = hs->cnt[0], P = hs->cnt[1];
    c->pipe.K = K;
    c->pipe.P = P;
    if (nInliers) *nInliers = P;
    if (stats) {
        stats_head(c, K, P, true, stats);
        float ms;
        hipEventElapsedTime(&ms, c->ev[EV_FRONT_START], c->ev[EV_END]);
        stats->total_ms = ms;
    }
}

// after a speculative front half (stage_descriptors' speculate): when the pack kernel flagged an
// element that is not an integer in [0, 255], the float rows (still on the device) go through the
// float matchers and the front half runs again, as the non-speculative staging would have run it
int redo_float_front(fm3d_ctx* c) {
    if (!c->specU8) return FM3D_OK;
    c->specU8 = false;
    const int flag = *c->hFlag.as<int>();
    if (flag == 0) return FM3D_OK;
    if (flag < 0) return fail(c, FM3D_ERR_HIP, "the float rows' flag never arrived");
    std::swap(c->A, c->fwd.q8);
    std::swap(c->B, c->fwd.t8);
    c->pipe.type = FM3D_DESC_F32;
    c->pipe.dimPad = c->pipe.dim;
    int r;
    if ((r = front_with_counts(c, true))) return r;
    HIPCHK(c, hipEventSynchronize(c->ev[EV_END]));
    return FM3D_OK;
}

// fm3d_pipeline_run(_dlt)_verified's argument rules, before any launch (haveRep: the call's report is not
// null, or it takes none; need: StagedIdle for a call on the staged pair, Idle for one that stages its own)
int check_verified(fm3d_ctx* c, const fm3d_verify_opts* o, bool haveRep, Need need = Need::StagedIdle) {
    if (!c || !o || !haveRep) return fail(c, FM3D_ERR_INVALID, "null argument");
    if (int r = require(c, need)) return r;
    if (o->hypotheses < 1) return fail(c, FM3D_ERR_INVALID, "hypotheses must be >= 1");
    if (o->refineIters < 0 || o->refineIters > 16) return fail(c, FM3D_ERR_INVALID, "refineIters must be in 0 .. 16");
    if (!good_max_px(o->maxPx)) return fail(c, FM3D_ERR_INVALID, "maxPx must be finite and > 0");
    if (o->reserved != 0) return fail(c, FM3D_ERR_INVALID, "reserved must be 0");
    if (o->poseFromModel != 0 && o->poseFromModel != 1) return fail(c, FM3D_ERR_INVALID, "poseFromModel must be 0 or 1");
    if (o->poseFromModel) {
        if (!good_max_px(o->baseline)) return fail(c, FM3D_ERR_INVALID, "baseline must be finite and > 0");
        if (c->s.guidedMatchPx > 0.)
            return fail(c, FM3D_ERR_INVALID,
                        "poseFromModel with guidedMatchPx > 0: the gate needs the pose this call is about to find");
    }
    if (need == Need::StagedIdle && c->pipe.queryOffset != 0)
        return fail(c, FM3D_ERR_UNSUPPORTED, "a staged queryOffset != 0: a share sees only its own matches");
    if (o->hypotheses > fm3d::kVerifyMaxHyps) return fail(c, FM3D_ERR_UNSUPPORTED, "more than 2^20 hypotheses");
    return FM3D_OK;
}

// The argument rules, the match half, one wait for K, the verification of those matches where they lie
// (verify_staged: its own wait), and the pose's installation.  *go: a model (and, when asked for, its
// pose) exists, the verified matches and their count are where front_dlt reads them.  Otherwise nothing
// further may be launched on this pair: its counts are zero on both sides, in *count and stats too.
int front_verified(fm3d_ctx* c, const fm3d_verify_opts* o, fm3d_verify_report* rep, int* count,
                   fm3d_pipeline_stats* stats, bool* go) {
    int r;
    *go = false;
    if ((r = check_verified(c, o, rep != nullptr))) return r;
    hipSetDevice(c->device);
    std::memset(rep, 0, sizeof(*rep));
    rep->best = -1;
    if ((r = front_match(c))) return r;
    int* cnt = c->pcnt.as<int>();
    int K = 0;
    HIPCHK(c, hipMemcpyAsync(&K, cnt + 0, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (K < 0 || K > c->pipe.nA) return fail(c, FM3D_ERR_HIP, "match count out of range");
    rep->matches = K;
    if (K >= 8) {  // fewer: no sample exists, every hypothesis is invalid
        bool havePose = false;
        double g[16];
        if ((r = verify_staged(c, o, K, rep, &havePose, g))) return r;
        *go = rep->best >= 0 && (!o->poseFromModel || havePose);
        if (*go && o->poseFromModel) {
            install_g12(c, g);
            rep->poseInstalled = 1;
        }
    }
    std::memcpy(rep->g12, c->g12, sizeof(rep->g12));
    if (!*go) {
        rep->verified = 0;
        for (int k = 0; k < 4; k++) rep->votes[k] = 0;
        c->pipe.K = c->pipe.P = 0;
        HIPCHK(c, hipMemsetAsync(cnt, 0, 4 * sizeof(int), c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (count) *count = 0;
        if (stats) stats_head(c, 0, 0, false, stats);  // no counts, no times
    }
    return FM3D_OK;
}

// the verified submits' rules on top: filter mode only, and no joined LM launches
int check_verified_submit(fm3d_ctx* c, const fm3d_verify_opts* o, Need need) {
    if (int r = check_verified(c, o, true, need)) return r;
    if (o->poseFromModel)
        return fail(c, FM3D_ERR_UNSUPPORTED,
                    "poseFromModel = 1 has no submit / wait form: the synchronous fm3d_pipeline_run_verified / "
                    "fm3d_pipeline_run_dlt_verified serve it");
    if (c->pipe.linkLeader || !c->pipe.linkMembers.empty())
        return fail(c, FM3D_ERR_UNSUPPORTED, "a linked context (fm3d_pipeline_link): verified pairs join no LM launch");
    return FM3D_OK;
}

// The verified path on the staged inputs, queued on the context stream: the match half, the
// verification on the device's counts with its compaction and the buffer swap (verify_staged_queue),
// then the DLT half with its counts to page-locked memory (front only) or the DLT, the LM, the records
// and the small D2H.  Nothing here waits for the device; with no model every later stage sees 0 items.
int enqueue_verified(fm3d_ctx* c, const fm3d_verify_opts* o, bool frontOnly) {
    int r;
    if ((r = front_match(c))) return r;
    if ((r = verify_staged_queue(c, o))) return r;
    if (frontOnly) return front_with_counts(c, false);
    if ((r = front_dlt(c, nullptr))) return r;
    return enqueue_normals(c, nullptr, &c->pipe.subLm);
}

}  // namespace

extern "C" {

int fm3d_pipeline_upload(fm3d_ctx* c, const void* descA, int nA, const void* descB, int nB, int dim, int type,
                         const fm3d_point2f* kpts1, const fm3d_point2f* kpts2, const uint8_t* img1, const uint8_t* img2,
                         int width, int height, int queryOffset) {
    int r;
    if ((r = require(c, Need::Idle))) return r;
    hipSetDevice(c->device);
    if ((r = stage_pipeline(c, {descA, nA, descB, nB, dim, type, kpts1, kpts2, img1, img2, width, height, queryOffset})))
        return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FM3D_OK;
}

int fm3d_pipeline_run(fm3d_ctx* c, fm3d_record* recordsDev, int* nKept, fm3d_pipeline_stats* stats) {
    int r;
    if ((r = require(c, Need::StagedIdle))) return r;
    hipSetDevice(c->device);
    fm3d_lm_stats ls{};
    if ((r = enqueue_full(c, recordsDev, &ls))) return r;
    return finalize_full(c, ls, c->ev[EV_FRONT_START], false, nKept, stats);
}

int fm3d_pipeline_submit(fm3d_ctx* c, const void* descA, int nA, const void* descB, int nB, int dim, int type,
                         const fm3d_point2f* kpts1, const fm3d_point2f* kpts2, const uint8_t* img1, const uint8_t* img2,
                         int width, int height, int queryOffset) {
    return submit_impl(c, {descA, nA, descB, nB, dim, type, kpts1, kpts2, img1, img2, width, height, queryOffset}, nullptr);
}

int fm3d_pipeline_link(fm3d_ctx* member, fm3d_ctx* leader) {
    if (!member || !leader || member == leader) return FM3D_ERR_INVALID;
    if (member->pipe.state != PairState::Idle || leader->pipe.state != PairState::Idle)
        return fail(member, FM3D_ERR_INVALID, "a submitted frame pair is pending");
    if (member->pipe.linkLeader || !member->pipe.linkMembers.empty() || leader->pipe.linkLeader)
        return fail(member, FM3D_ERR_INVALID, "a context is linked already");
    if ((int)leader->pipe.linkMembers.size() + 1 >= fm3d::kLMMaxProblems)
        return fail(member, FM3D_ERR_INVALID, "a leader takes at most 3 members");
    if (member->device != leader->device) return fail(member, FM3D_ERR_INVALID, "linked contexts need one device");
    member->pipe.linkLeader = leader;
    leader->pipe.linkMembers.push_back(member);
    return FM3D_OK;
}

int fm3d_pipeline_wait(fm3d_ctx* c, fm3d_record* out, int cap, int* nKept, fm3d_pipeline_stats* stats) {
    int r;
    if ((r = require(c, Need::Full))) return r;
    hipSetDevice(c->device);
    if ((r = flush_member(c))) return r;
    c->pipe.state = PairState::Idle;
    int kept = 0;
    if ((r = finalize_full(c, c->pipe.subLm, c->ev[EV_SUBMIT_START], true, &kept, stats))) return r;
    if (out && kept > cap) return fail(c, FM3D_ERR_INVALID, "record buffer too small");
    if (out && kept)
        HIPCHK(c, hipMemcpy(out, c->pipe.pendOut, (size_t)kept * sizeof(fm3d_record), hipMemcpyDeviceToHost));
    if (nKept) *nKept = kept;
    return FM3D_OK;
}

int fm3d_pipeline_submit_dlt(fm3d_ctx* c) {
    int r;
    if ((r = require(c, Need::StagedIdle))) return r;
    hipSetDevice(c->device);
    if ((r = front_with_counts(c, true))) return r;
    c->pipe.state = PairState::DltFront;
    return FM3D_OK;
}

int fm3d_pipeline_submit_dlt_pair(fm3d_ctx* c, const void* descA, int nA, const void* descB, int nB, int dim,
                                  int type, const fm3d_point2f* kpts1, const fm3d_point2f* kpts2, int queryOffset) {
    int r;
    if ((r = require(c, Need::Idle))) return r;
    hipSetDevice(c->device);
    if ((r = stage_pipeline(c, {descA, nA, descB, nB, dim, type, kpts1, kpts2, nullptr, nullptr, 0, 0, queryOffset}, true)))
        return r;
    if ((r = front_with_counts(c, true))) return r;
    c->pipe.state = PairState::DltFront;
    return FM3D_OK;
}

int fm3d_pipeline_wait_dlt(fm3d_ctx* c, int* nInliers, fm3d_pipeline_stats* stats) {
    int r;
    if ((r = require(c, Need::Dlt))) return r;
    hipSetDevice(c->device);
    c->pipe.state = PairState::Idle;
    HIPCHK(c, hipEventSynchronize(c->ev[EV_END]));
    if ((r = redo_float_front(c))) return r;
    report_front_counts(c, nInliers, stats);
    return FM3D_OK;
}

int fm3d_pipeline_run_dlt(fm3d_ctx* c, int* nInliers, fm3d_pipeline_stats* stats) {
    if (int r = fm3d_pipeline_submit_dlt(c)) return r;
    return fm3d_pipeline_wait_dlt(c, nInliers, stats);
}

int fm3d_pipeline_run_verified(fm3d_ctx* c, const fm3d_verify_opts* o, fm3d_record* recordsDev, int* nKept,
                               fm3d_pipeline_stats* stats, fm3d_verify_report* rep) {
    int r;
    bool go;
    if ((r = front_verified(c, o, rep, nKept, stats, &go)) || !go) return r;
    fm3d_lm_stats ls{};
    if ((r = front_dlt(c, nullptr))) return r;
    if ((r = enqueue_normals(c, recordsDev, &ls))) return r;
    return finalize_full(c, ls, c->ev[EV_FRONT_START], false, nKept, stats);
}

int fm3d_pipeline_run_dlt_verified(fm3d_ctx* c, const fm3d_verify_opts* o, int* nInliers, fm3d_pipeline_stats* stats,
                                   fm3d_verify_report* rep) {
    int r;
    bool go;
    if ((r = front_verified(c, o, rep, nInliers, stats, &go)) || !go) return r;
    if ((r = front_with_counts(c, false))) return r;
    HIPCHK(c, hipEventSynchronize(c->ev[EV_END]));
    report_front_counts(c, nInliers, stats);
    return FM3D_OK;
}

int fm3d_pipeline_submit_verified(fm3d_ctx* c, const fm3d_verify_opts* o, const void* descA, int nA, const void* descB,
                                  int nB, int dim, int type, const fm3d_point2f* kpts1, const fm3d_point2f* kpts2,
                                  const uint8_t* img1, const uint8_t* img2, int width, int height) {
    int r;
    if ((r = check_verified_submit(c, o, Need::Idle))) return r;
    hipSetDevice(c->device);
    HIPCHK(c, hipEventRecord(c->ev[EV_SUBMIT_START], c->stream));
    if ((r = stage_pipeline(c, {descA, nA, descB, nB, dim, type, kpts1, kpts2, img1, img2, width, height, 0}))) return r;
    c->pipe.subLm = fm3d_lm_stats{};
    c->pipe.subOut = nullptr;
    if ((r = enqueue_verified(c, o, false))) return r;
    c->pipe.state = PairState::Verified;
    return FM3D_OK;
}

int fm3d_pipeline_wait_verified(fm3d_ctx* c, fm3d_record* out, int cap, int* nKept, fm3d_pipeline_stats* stats,
                                fm3d_verify_report* rep) {
    int r;
    if (!c || !rep) return fail(c, FM3D_ERR_INVALID, "null argument");
    if ((r = require(c, Need::Verified))) return r;
    hipSetDevice(c->device);
    c->pipe.state = PairState::Idle;
    int kept = 0;
    if ((r = finalize_full(c, c->pipe.subLm, c->ev[EV_SUBMIT_START], true, &kept, stats))) return r;
    if ((r = verify_report(c, rep))) return r;
    if (out && kept > cap) return fail(c, FM3D_ERR_INVALID, "record buffer too small");
    if (out && kept)
        HIPCHK(c, hipMemcpy(out, c->pipe.pendOut, (size_t)kept * sizeof(fm3d_record), hipMemcpyDeviceToHost));
    if (nKept) *nKept = kept;
    return FM3D_OK;
}

int fm3d_pipeline_submit_dlt_verified(fm3d_ctx* c, const fm3d_verify_opts* o) {
    int r;
    if ((r = check_verified_submit(c, o, Need::StagedIdle))) return r;
    hipSetDevice(c->device);
    if ((r = enqueue_verified(c, o, true))) return r;
    c->pipe.state = PairState::DltVerified;
    return FM3D_OK;
}

int fm3d_pipeline_wait_dlt_verified(fm3d_ctx* c, int* nInliers, fm3d_pipeline_stats* stats, fm3d_verify_report* rep) {
    int r;
    if (!c || !rep) return fail(c, FM3D_ERR_INVALID, "null argument");
    if ((r = require(c, Need::DltVerified))) return r;
    hipSetDevice(c->device);
    c->pipe.state = PairState::Idle;
    HIPCHK(c, hipEventSynchronize(c->ev[EV_END]));
    if ((r = verify_report(c, rep))) return r;
    report_front_counts(c, nInliers, stats);
    return FM3D_OK;
}

int fm3d_pipeline_submit_ncc(fm3d_ctx* c, int Hphi, int Htheta, double span) {
    int r;
    if ((r = require(c, Need::StagedIdle))) return r;
    if (Hphi <= 0 || Htheta <= 0 || Hphi * Htheta > 32) return fail(c, FM3D_ERR_INVALID, "1 <= Hphi * Htheta <= 32");
    if (!c->haveG12) return fail(c, FM3D_ERR_INVALID, "fm3d_set_g12 / fm3d_setg12 not called");
    hipSetDevice(c->device);
    c->nccP = 0;
    if ((r = pipeline_front(c))) return r;
    const int nA = c->pipe.nA;
    const int H = Hphi * Htheta;
    HIPCHK(c, hipEventRecord(c->ev[EV_NORMAL_START], c->stream));
    if (nA > 0) {
        if ((r = ensure_offsets(c))) return r;
        HIPCHK(c, c->nccS.ensure((size_t)nA * H * sizeof(double)));
        HIPCHK(c, c->nccN.ensure((size_t)nA * 3 * sizeof(double)));
        HIPCHK(c, c->nccB.ensure((size_t)nA * sizeof(int)));
        fm3d::NccParams p = ncc_params(c, Hphi, Htheta, span);
        p.points = c->pts.as<double>();
        p.P = nA;  // the bound; the inlier count is on the device
        p.Pdev = c->pcnt.as<int>() + 1;
        p.scores = c->nccS.as<double>();
        p.normals = c->nccN.as<double>();
        p.best = c->nccB.as<int>();
        fm3d::launch_ncc_hypotheses(p, c->stream);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipEventRecord(c->ev[EV_NORMAL_END], c->stream));
    HIPCHK(c, c->hSmall.ensure(sizeof(PipeSmall)));
    PipeSmall* hs = c->hSmall.as<PipeSmall>();
    HIPCHK(c, hipMemcpyAsync(hs->cnt, c->pcnt.p, sizeof(hs->cnt), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(c->ev[EV_END], c->stream));
    c->pipe.state = PairState::Ncc;
    c->pipe.nccHPending = H;
    return FM3D_OK;
}

int fm3d_pipeline_wait_ncc(fm3d_ctx* c, int* nPoints, fm3d_pipeline_stats* stats) {
    if (int r = require(c, Need::Ncc)) return r;
    hipSetDevice(c->device);
    c->pipe.state = PairState::Idle;
    HIPCHK(c, hipEventSynchronize(c->ev[EV_END]));
    const PipeSmall* hs = c->hSmall.as<PipeSmall>();
    const int K = hs->cnt[0], P = hs->cnt[1];
    c->pipe.K = K;
    c->pipe.P = P;
    c->nccH = c->pipe.nccHPending;
    c->nccP = P;  // the score rows fm3d_pipeline_ncc_download returns (set only by a successful run)
    if (nPoints) *nPoints = P;
    if (stats) {
        stats_head(c, K, P, true, stats);
        stats->kept = P;
        float ms;
        hipEventElapsedTime(&ms, c->ev[EV_NORMAL_START], c->ev[EV_NORMAL_END]);
        stats->lm_ms = ms;  // the normal stage: here the NCC scoring
        hipEventElapsedTime(&ms, c->ev[EV_FRONT_START], c->ev[EV_END]);
        stats->total_ms = ms;
    }
    return FM3D_OK;
}

int fm3d_pipeline_run_ncc(fm3d_ctx* c, int Hphi, int Htheta, double span, int* nPoints, fm3d_pipeline_stats* stats) {
    if (int r = fm3d_pipeline_submit_ncc(c, Hphi, Htheta, span)) return r;
    return fm3d_pipeline_wait_ncc(c, nPoints, stats);
}

int fm3d_pipeline_ncc_download(fm3d_ctx* c, double* scores, double* normals, int32_t* best) {
    if (!c || !c->staged) return FM3D_ERR_INVALID;
    if (int r = require(c, Need::Idle)) return r;
    hipSetDevice(c->device);
    // the rows of the last successful fm3d_pipeline_run_ncc (a later run / run_dlt does not resize them)
    const size_t P = (size_t)c->nccP;
    if (P && scores) HIPCHK(c, hipMemcpy(scores, c->nccS.p, P * c->nccH * sizeof(double), hipMemcpyDeviceToHost));
    if (P && normals) HIPCHK(c, hipMemcpy(normals, c->nccN.p, P * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (P && best) HIPCHK(c, hipMemcpy(best, c->nccB.p, P * sizeof(int), hipMemcpyDeviceToHost));
    return FM3D_OK;
}

int fm3d_pipeline_dlt_download(fm3d_ctx* c, fm3d_dmatch* matches, double* points, int32_t* matchIdx) {
    if (!c || !c->staged) return FM3D_ERR_INVALID;
    if (int r = require(c, Need::Idle)) return r;
    hipSetDevice(c->device);
    if (matches && c->pipe.K) HIPCHK(c, hipMemcpy(matches, c->matches.p, (size_t)c->pipe.K * sizeof(fm3d_dmatch), hipMemcpyDeviceToHost));
    if (points && c->pipe.P) HIPCHK(c, hipMemcpy(points, c->pts.p, (size_t)c->pipe.P * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (matchIdx && c->pipe.P) HIPCHK(c, hipMemcpy(matchIdx, c->srcIdx.p, (size_t)c->pipe.P * sizeof(int), hipMemcpyDeviceToHost));
    return FM3D_OK;
}

}  // extern "C"

// ---- internal entry points of the multi-GPU host (fm3d_mgpu.cpp; fm3d_internal.h, not the C ABI)
int fm3d_internal_submit_to(fm3d_ctx* c, const void* descA, int nA, const void* descB, int nB, int dim, int type,
                            const fm3d_point2f* kpts1, const fm3d_point2f* kpts2, const uint8_t* img1,
                            const uint8_t* img2, int width, int height, fm3d_record* recordsDev) {
    return submit_impl(c, {descA, nA, descB, nB, dim, type, kpts1, kpts2, img1, img2, width, height, 0}, recordsDev);
}

int fm3d_internal_flush(fm3d_ctx* c) { return c ? flush_member(c) : FM3D_ERR_INVALID; }
bool fm3d_internal_front_only(const fm3d_ctx* c) { return c && c->pipe.state == PairState::MemberFront; }

int fm3d_internal_enqueue(fm3d_ctx* c, fm3d_record* recordsDev) {
    int r;
    if ((r = require(c, Need::StagedIdle))) return r;
    hipSetDevice(c->device);
    HIPCHK(c, hipEventRecord(c->ev[EV_SUBMIT_START], c->stream));
    c->pipe.subLm = fm3d_lm_stats{};
    if ((r = enqueue_full(c, recordsDev, &c->pipe.subLm))) return r;
    c->pipe.state = PairState::Full;
    return FM3D_OK;
}

int fm3d_internal_finish(fm3d_ctx* c, int* nKept, fm3d_pipeline_stats* stats) {
    if (!c || c->pipe.state == PairState::Idle) return fail(c, FM3D_ERR_INVALID, "nothing pending");
    hipSetDevice(c->device);
    c->pipe.state = PairState::Idle;
    return finalize_full(c, c->pipe.subLm, c->ev[EV_SUBMIT_START], true, nKept, stats);
}

const int* fm3d_internal_kept_dev(fm3d_ctx* c) { return c->pcnt.as<int>() + 2; }
hipStream_t fm3d_internal_stream(fm3d_ctx* c) { return c->stream; }
// the device memory one context may take: its largest LM launch's slabs (every CU filled) plus the
// per-pair buffers of nA queries against nB train rows of dim elements (a conservative estimate of
// what the pipeline's DevBufs grow to: descriptors, their u8 / unpacked copies, per-query match,
// triangulation, LM and record arrays, the matchers' part lists, pyramids)
int fm3d_internal_memory_need(fm3d_ctx* c, int64_t nA, int64_t nB, int dim, int type, int width, int height,
                              size_t* bytes) {
    hipSetDevice(c->device);
    int r;
    if ((r = ensure_offsets(c))) return r;
    const bool tree = c->s.lmReduction != 0;
    const int slots = fm3d::kLM2Slots + (tree ? 1 : 0);
    const void* kptr = tree ? reinterpret_cast<const void*>(fm3d::lm2_kernel<true, true, false>)
                            : reinterpret_cast<const void*>(fm3d::lm2_kernel<true, false, false>);
    long groups = 0;
    if ((r = lm_groups(c, kptr, slots, -1, &groups))) return r;
    const size_t ents = (size_t)c->nOffPad * slots;
    size_t need = ents * (2 * sizeof(double) + 5 * 4) * groups + 32768;
    const size_t rowIn = type == FM3D_DESC_F32 ? (size_t)dim * 4 : (size_t)dim;
    const size_t rowWork = 256 + (type == FM3D_DESC_F32 ? (size_t)dim * 4 : 0);  // u8 / unpacked / pair copies
    need += (size_t)(nA + nB) * (rowIn + rowWork) + (size_t)nB * 64;
    if (c->s.guidedMatchPx > 0.) need += (size_t)nA * 16 + (size_t)nB * 8;  // the gate's lines and (u, v)
    // the cross-check's reverse search: unpacked / pair copies of both sides, row constants, the
    // train rows' top-2 lists and 16 parts of them
    if (c->s.crossCheck != 0) need += (size_t)(nA + nB) * (rowWork + 8) + (size_t)nB * (24 + 16 * 16);
    need += (size_t)nA * 1536;  // per query: top-2 lists + 16 parts, matches, points, masks, LM arrays, records
    need += (size_t)width * height * 4 + ((size_t)16 << 20);  // pyramids with guards, small buffers
    // image 2's column-major levels: level 0's (w + 2) columns of stride <= h + 65, the others a third more
    need += (size_t)(width + 2) * (height + 65) * 2;
    *bytes = need;
    return FM3D_OK;
}

int fm3d_internal_alloc_probe(fm3d_ctx* c, size_t bytes, uint8_t* out) {
    if (!c || !bytes || !out) return fail(c, FM3D_ERR_INVALID, "alloc_probe: null context, no bytes or null out");
    hipSetDevice(c->device);
    DevBuf b;
    HIPCHK(c, b.ensure(bytes));
    HIPCHK(c, hipMemcpy(out, b.p, bytes, hipMemcpyDeviceToHost));
    return FM3D_OK;
}

int fm3d_internal_prepare(fm3d_ctx* c) {  // the device count buffer, before a collective names it
    hipSetDevice(c->device);
    HIPCHK(c, c->pcnt.ensure(64));
    return FM3D_OK;
}
