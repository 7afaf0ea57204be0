// schedule.cc — schedule IR generators (see schedule.h).
//
// Association orders, per element, with "acc = src (op) acc" as in LocalReduce:
//   one-shot AllReduce, mesh ReduceScatter, Reduce   O1: acc = x_me, then x_r for r ascending, r != me
//       ins_temp_all_reduce_mesh_1D_one_shot.cc:211-226, ins_temp_reduce_scatter_mesh_1D.cc:165-203,
//       reduce_mesh_1D.cc:232-246, reduce_mesh_1D_two_shot.cc:226-247
//   two-shot AllReduce                               O2: acc = x_0, then x_1 .. x_{n-1}
//       ins_temp_all_reduce_mesh_1D_two_shot.cc:312-338
//   rings (build-side; the reference has no ring AllReduce template): R arc-disjoint Hamiltonian cycles, part k on
//       ring k; chunk at position c: acc = x_{cyc[c+1]}, then x_{cyc[c+2]} .. x_{cyc[c]}
//   RHD (docs/zh/user_guide/coll_algo_intro/RHD.md)  pairwise tree, partner = rank ^ d, d = n/2, n/4, .., 1
//   NHR AllReduce                                    O5: ins_temp_all_reduce_nhr.cc:230-301, 390-482
//
// Data movement: a rank's data leaves it through SEND/RECV records grouped into one RCCL group per pipeline step;
// every schedule is cut into pieces ("pipelining granule") so that the transfer of piece t+1 overlaps the reduce
// of piece t, and the staging ("CCL buffer", SCRATCH) holds only a bounded number of pieces. The executor derives
// every cross-stream dependency from the byte ranges the records touch, so the generators only have to emit a
// correct program order.
#include "schedule.h"

#include <algorithm>

namespace hccl_amd {

namespace {

constexpr uint64_t kAlignBytes = 128;  // HCCL_MIN_SLICE_ALIGN, alg_template_base.h:34
constexpr uint64_t kOneShotMaxBytes = 8ull << 20;

struct Ref {
    int32_t buf;
    uint64_t off;
};

class Builder {
public:
    std::vector<HcclAmdIrOp> ops;
    uint64_t scratchHigh = 0;
    int32_t group = 0;
    // Element offset added to every INPUT / OUTPUT reference: a generator written for [0, count) then runs one
    // executor loop [ioBase, ioBase + count) of the reference's OrchestrateLoop.
    uint64_t ioBase = 0;

    void Copy(Ref dst, Ref src, uint64_t count)
    {
        if (count == 0) return;
        HcclAmdIrOp o = Blank(HCCL_AMD_IR_COPY, count);
        SetDst(o, dst, count);
        AddSrc(o, src, count);
        ops.push_back(o);
    }
    void Reduce(Ref dst, const std::vector<Ref>& srcs, uint64_t count)
    {
        if (count == 0) return;
        HcclAmdIrOp o = Blank(HCCL_AMD_IR_REDUCE, count);
        SetDst(o, dst, count);
        for (const Ref& s : srcs) AddSrc(o, s, count);
        ops.push_back(o);
    }
    void Send(uint32_t peer, Ref src, uint64_t count)
    {
        if (count == 0) return;
        HcclAmdIrOp o = Blank(HCCL_AMD_IR_SEND, count);
        o.peer = static_cast<int32_t>(peer);
        o.group = group;
        AddSrc(o, src, count);
        ops.push_back(o);
    }
    void Recv(uint32_t peer, Ref dst, uint64_t count)
    {
        if (count == 0) return;
        HcclAmdIrOp o = Blank(HCCL_AMD_IR_RECV, count);
        o.peer = static_cast<int32_t>(peer);
        o.group = group;
        SetDst(o, dst, count);
        ops.push_back(o);
    }
    void EndGroup() { group++; }

private:
    static HcclAmdIrOp Blank(int32_t kind, uint64_t count)
    {
        HcclAmdIrOp o{};
        o.kind = kind;
        o.peer = -1;
        o.nsrc = 0;
        o.group = -1;
        o.count = count;
        o.dstBuf = -1;
        for (int i = 0; i < HCCL_AMD_IR_MAX_SRC; ++i) o.srcBuf[i] = -1;
        return o;
    }
    void Track(Ref r, uint64_t count)
    {
        if (r.buf == HCCL_AMD_BUF_SCRATCH) scratchHigh = std::max(scratchHigh, r.off + count);
    }
    uint64_t Base(Ref r) const { return r.buf == HCCL_AMD_BUF_SCRATCH ? r.off : r.off + ioBase; }
    void SetDst(HcclAmdIrOp& o, Ref r, uint64_t count)
    {
        o.dstBuf = r.buf;
        o.dstOff = Base(r);
        Track(r, count);
    }
    void AddSrc(HcclAmdIrOp& o, Ref r, uint64_t count)
    {
        o.srcBuf[o.nsrc] = r.buf;
        o.srcOff[o.nsrc] = Base(r);
        o.nsrc++;
        Track(r, count);
    }
};

uint64_t AlignUp(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }
uint64_t CeilDiv(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

// Elements per 128-B slice alignment unit (at least one).
uint64_t AlignElems(const ScheduleParams& p) { return std::max<uint64_t>(1, kAlignBytes / p.elemSize); }

// Pieces of pe elements that cover `len` elements; at least one, so that every rank posts the same groups.
uint64_t NumPieces(uint64_t len, uint64_t pe) { return std::max<uint64_t>(1, CeilDiv(len, pe)); }

// A contiguous element range [begin, begin + len).
struct Span {
    uint64_t begin;
    uint64_t len;
};

// Chunk c of n for a buffer of `count` elements: ceil(count / n) rounded up to the 128-B slice alignment
// (two-shot slicing, ins_temp_all_reduce_mesh_1D_two_shot.cc:170-202, with HCCL_MIN_SLICE_ALIGN); trailing chunks
// may be short or empty.
Span Chunk(uint64_t count, uint32_t n, uint32_t c, uint64_t alignElems)
{
    uint64_t sc = AlignUp(CeilDiv(count, n), alignElems);
    uint64_t b = std::min<uint64_t>(count, uint64_t(c) * sc);
    uint64_t e = std::min<uint64_t>(count, b + sc);
    return {b, e - b};
}

// The reference's executor loop (InsV2AllReduceSoleExecutor::OrchestrateLoop,
// ins_v2_all_reduce_sole_executor.cc:160-208; ReduceSoleExecutor, reduce_sole_executor.cc:120-170): at most
// min(transportBound, ccl / scratchMultiple rounded down to 128 B) bytes per loop, and the template slices each loop's
// data on its own. Orders that depend on which rank owns an element (NHR, Reduce two-shot) therefore follow these
// loops. ccl = HCCL_BUFFSIZE (the reference's simulator and default: 200 MB).
constexpr uint64_t kUbMaxDataSize = 256ull << 20;  // UB_MAX_DATA_SIZE, alg_param.h:37

uint64_t RefLoopElems(const ScheduleParams& p, uint64_t transportBoundBytes, uint64_t scratchMultiple)
{
    const uint64_t ccl = p.cclBytes;
    uint64_t bytes = transportBoundBytes;
    if (scratchMultiple != 0) bytes = std::min(bytes, ccl / scratchMultiple / kAlignBytes * kAlignBytes);
    return std::max<uint64_t>(1, bytes / p.elemSize);
}

// Runs gen(loopParams) once per executor loop, with the builder's I/O base at the loop's first element.
template <class Gen>
void ForEachRefLoop(const ScheduleParams& p, Builder& b, uint64_t loopElems, Gen gen)
{
    for (uint64_t off = 0; off < p.count; off += loopElems) {
        ScheduleParams lp = p;
        lp.count = std::min(loopElems, p.count - off);
        b.ioBase = off;
        gen(lp);
    }
    b.ioBase = 0;
}

// ReduceMesh1DTwoShot::CalcSlice (reduce_mesh_1D_two_shot.cc:108-131): the first count % n ranks get one element more.
Span BalancedSlice(uint64_t count, uint32_t n, uint32_t c)
{
    const uint64_t base = count / n, rem = count % n;
    return {uint64_t(c) * base + std::min<uint64_t>(c, rem), base + (c < rem ? 1 : 0)};
}

// ReduceNHR::CalcSlice (reduce_nhr.cc:114-138): chunk = RoundUpWithDivisor(bytes, n * elemSize) / n, i.e.
// ceil(count / n) elements; trailing slices short or empty.
Span CeilSlice(uint64_t count, uint32_t n, uint32_t c) { return Chunk(count, n, c, 1); }

// InsTempAllReduceNHR::KernelRun (ins_temp_all_reduce_nhr.cc:171-173): floor(count / n), the tail on the last slice.
Span FloorSlice(uint64_t count, uint32_t n, uint32_t c)
{
    const uint64_t se = count / n;
    return c == n - 1 ? Span{uint64_t(c) * se, count - se * (n - 1)} : Span{uint64_t(c) * se, se};
}

// Piece p of a span cut into pieces of pe elements (the last may be short, those past the end are empty).
Span Piece(Span s, uint64_t pe, uint64_t p)
{
    uint64_t b = std::min<uint64_t>(s.len, p * pe);
    uint64_t e = std::min<uint64_t>(s.len, b + pe);
    return {s.begin + b, e - b};
}

// Granule choice: the requested piece size, else about a quarter of the per-peer slice within [256 KiB, 16 MiB];
// then shrunk until `slotsNeeded` staging pieces fit the scratch capacity.
uint64_t PieceElems(const ScheduleParams& p, uint64_t sliceElems, uint64_t slotsNeeded)
{
    const uint64_t es = p.elemSize;
    const uint64_t alignElems = AlignElems(p);
    uint64_t bytes = p.pieceBytes;
    if (bytes == 0) {
        bytes = std::clamp<uint64_t>(sliceElems * es / 4, 256ull << 10, 16ull << 20);
    }
    if (p.scratchCapBytes != 0 && slotsNeeded != 0) {
        uint64_t capPer = p.scratchCapBytes / slotsNeeded;
        capPer = capPer / kAlignBytes * kAlignBytes;
        if (capPer == 0) capPer = kAlignBytes;
        bytes = std::min(bytes, capPer);
    }
    return std::max<uint64_t>(alignElems, bytes / es / alignElems * alignElems);
}

Ref In(uint64_t off) { return {HCCL_AMD_BUF_INPUT, off}; }
Ref Out(uint64_t off) { return {HCCL_AMD_BUF_OUTPUT, off}; }
Ref Scr(uint64_t off) { return {HCCL_AMD_BUF_SCRATCH, off}; }

// Peer visiting order for mesh steps: me+1, me+2, ... (each rank starts on a different link).
std::vector<uint32_t> PeerOrder(uint32_t n, uint32_t me)
{
    std::vector<uint32_t> v;
    for (uint32_t i = 1; i < n; ++i) v.push_back((me + i) % n);
    return v;
}

// Index of peer q among the n-1 peers in ascending rank order (slot layout of the staging area).
uint32_t PeerSlot(uint32_t q, uint32_t me) { return q < me ? q : q - 1; }

// Staging slots of pe elements from element `base` of the staging: `depth` sets of `width` slots each, pipeline unit
// u using set u % depth. A generator's staging need is base + depth * width * pe elements.
struct SlotRing {
    uint64_t base, depth, width, pe;
    Ref At(uint64_t unit, uint64_t idx) const { return Scr(base + ((unit % depth) * width + idx) * pe); }
    // slotOf(q) of a unit whose set has one slot per peer of `me` (width n-1)
    auto Peers(uint64_t unit, uint32_t me) const
    {
        return [*this, unit, me](uint32_t q) { return At(unit, PeerSlot(q, me)); };
    }
};

// One end of a transfer: `len` elements at `ref`.
struct Seg {
    Ref ref;
    uint64_t len;
};

// Mesh exchange with every peer in PeerOrder: sendOf(q) goes to q, recvOf(q) comes from q. The caller ends the group.
template <class SendOf, class RecvOf>
void MeshExchange(Builder& b, uint32_t n, uint32_t me, SendOf sendOf, RecvOf recvOf)
{
    for (uint32_t q : PeerOrder(n, me)) {
        const Seg s = sendOf(q), r = recvOf(q);
        b.Send(q, s.ref, s.len);
        b.Recv(q, r.ref, r.len);
    }
}

// Reduce-scatter half of a mesh step, pieceOf(q) = this step's piece of the chunk rank q owns: my input of q's piece
// goes to q, and q's input of my piece arrives in slotOf(q).
template <class PieceOf, class SlotOf>
void ScatterPieces(Builder& b, uint32_t n, uint32_t me, PieceOf pieceOf, SlotOf slotOf)
{
    const uint64_t mine = pieceOf(me).len;
    MeshExchange(
        b, n, me,
        [&](uint32_t q) {
            const Span out = pieceOf(q);
            return Seg{In(out.begin), out.len};
        },
        [&](uint32_t q) { return Seg{slotOf(q), mine}; });
}

// All-gather half: my reduced piece in recvBuf goes to every peer, theirs arrive at their place in recvBuf.
template <class PieceOf>
void GatherPieces(Builder& b, uint32_t n, uint32_t me, PieceOf pieceOf)
{
    const Span mine = pieceOf(me);
    MeshExchange(
        b, n, me, [&](uint32_t) { return Seg{Out(mine.begin), mine.len}; },
        [&](uint32_t q) {
            const Span theirs = pieceOf(q);
            return Seg{Out(theirs.begin), theirs.len};
        });
}

// O1 operand list: own operand, then the peers' slots in ascending rank order, skipping me.
template <class SlotOf>
std::vector<Ref> O1Srcs(Ref own, uint32_t n, uint32_t me, SlotOf slotOf)
{
    std::vector<Ref> srcs{own};
    for (uint32_t q = 0; q < n; ++q) {
        if (q != me) srcs.push_back(slotOf(q));
    }
    return srcs;
}

// Two-shot pipeline over nu units: step u posts the scatter of unit u together with the gather of unit u-2 in one
// group, so the fold of unit u-1 runs while both transfers are on the links; then it folds unit u.
template <class Scatter, class Gather, class Fold>
void TwoShotPipeline(Builder& b, uint64_t nu, Scatter scatter, Gather gather, Fold fold)
{
    for (uint64_t u = 0; u < nu + 2; ++u) {
        if (u < nu) scatter(u);
        if (u >= 2) gather(u - 2);
        b.EndGroup();
        if (u < nu) fold(u);
    }
}

// ------------------------------------------------------------------------------------------- AllReduce

// One-shot (O1): every rank sends its whole input to every peer; each rank folds own + peers ascending.
void AllReduceOneShot(const ScheduleParams& p, Builder& b)
{
    const uint32_t n = p.nRanks, me = p.rank;
    const SlotRing slots{0, 2, n - 1, PieceElems(p, p.count, 2 * (n - 1))};
    const uint64_t np = CeilDiv(p.count, slots.pe);
    for (uint64_t t = 0; t < np; ++t) {
        const Span s = Piece({0, p.count}, slots.pe, t);
        const auto slot = slots.Peers(t, me);
        ScatterPieces(b, n, me, [&](uint32_t) { return s; }, slot);  // every "chunk" is the whole piece
        b.EndGroup();
        b.Reduce(Out(s.begin), O1Srcs(In(s.begin), n, me, slot), s.len);
    }
}

// The two-shot structure: mesh reduce-scatter of n chunks (ceil(count / n) rounded up to 128 B) into two sets of
// staging slots, one slot per peer or, with `ownSlot`, one per rank; fold(piece of my chunk, slotOf) writes the reduced
// piece to recvBuf; mesh all-gather. Pieces run through TwoShotPipeline.
template <class Fold>
void AllReduceTwoShotWith(const ScheduleParams& p, Builder& b, bool ownSlot, Fold fold)
{
    const uint32_t n = p.nRanks, me = p.rank;
    const uint64_t maxChunk = Chunk(p.count, n, 0, AlignElems(p)).len, width = ownSlot ? n : n - 1;
    const SlotRing slots{0, 2, width, PieceElems(p, maxChunk, 2 * width)};
    auto piece = [&](uint64_t t) {
        return [&p, n, pe = slots.pe, t](uint32_t q) { return Piece(Chunk(p.count, n, q, AlignElems(p)), pe, t); };
    };
    auto slot = [&](uint64_t t) {
        return [=](uint32_t q) { return slots.At(t, ownSlot ? q : PeerSlot(q, me)); };
    };
    TwoShotPipeline(
        b, NumPieces(maxChunk, slots.pe), [&](uint64_t t) { ScatterPieces(b, n, me, piece(t), slot(t)); },
        [&](uint64_t g) { GatherPieces(b, n, me, piece(g)); }, [&](uint64_t t) { fold(piece(t)(me), slot(t)); });
}

// Two-shot (O2): fold of chunk `me` in rank order 0..n-1, the own operand from the input.
void AllReduceTwoShot(const ScheduleParams& p, Builder& b)
{
    const uint32_t n = p.nRanks, me = p.rank;
    AllReduceTwoShotWith(p, b, false, [&](Span rs, auto slotOf) {
        std::vector<Ref> srcs;
        for (uint32_t q = 0; q < n; ++q) srcs.push_back(q == me ? In(rs.begin) : slotOf(q));
        b.Reduce(Out(rs.begin), srcs, rs.len);
    });
}

// ------------------------------------------------------------------------------------------- MeshChunk (O6)
//
// The reference's MeshChunk templates (ins_temp_all_reduce_mesh_1D_two_shot_mesh_chunk.cc:161-275,
// ins_temp_reduce_scatter_mesh_1D_meshchunk.cc:139-252) cut the chunk that rank t owns into n-1 sub-slices and run
// n-1 steps; in step s every rank write-reduces its raw input of sub-slice i of peer (me - nextNum)'s chunk into
// that peer's CCL buffer, nextNum = s + i + 1, plus one when it reaches n (:207-212 / :200-204). Receiver t thus
// gets sub-slice j at step s from sender t + f(s + j + 1), f(x) = x < n ? x : x + 1. Writes into one receiver are
// serialised step by step: a sender waits for the receiver's ACK of step s+1, which the receiver posts only after all
// of its threads have seen the DATA signals of step s and synchronised (PostSyncInterThreads / PreSyncInterThreads,
// :264-273; SendRecvBatchWriteReduce's handshake, alg_data_trans_wrapper.cc:247-272, 481-514). The CCL buffer starts
// as the receiver's own input (PreCopy), so sub-slice j of owner t is the left fold
//     acc = x_t;  acc = x_{t+o} (op) acc  for o = j+1, ..., n-1, 1, ..., j   (peers by rank offset, mod n)  — O6.
// Here the raw inputs are exchanged into staging slots (as in the two-shot) and every (piece, sub-slice) segment is
// one ordered n-ary fold with that operand order; the data movement granule does not affect the bits.

// Sub-slices of a chunk of `count` elements, AllReduce form (…mesh_chunk.cc:166-183): n-1 slices, the first
// count % (n-1) one element longer.
std::vector<Span> SubSlicesEven(uint64_t count, uint32_t parts)
{
    std::vector<Span> v;
    const uint64_t base = count / parts, big = count % parts;
    uint64_t b = 0;
    for (uint32_t i = 0; i < parts; ++i) {
        const uint64_t len = base + (i < big ? 1 : 0);
        v.push_back({b, len});
        b += len;
    }
    return v;
}

// ReduceScatter form (…meshchunk.cc:155-180): n-2 slices of floor(bytes / (n-1)) rounded down to AICPU_ALIGN_SIZE
// (4 KiB, alg_param.h:91) and the remainder last; the even split when that alignment leaves nothing.
std::vector<Span> SubSlicesRs(uint64_t count, uint32_t parts, uint32_t es)
{
    constexpr uint64_t kAicpuAlign = 4096;
    const uint64_t align = count * es / parts / kAicpuAlign * kAicpuAlign;
    if (parts < 2 || align == 0) return SubSlicesEven(count, parts);
    std::vector<Span> v;
    const uint64_t a = align / es;
    for (uint32_t i = 0; i + 1 < parts; ++i) v.push_back({uint64_t(i) * a, a});
    v.push_back({uint64_t(parts - 1) * a, count - uint64_t(parts - 1) * a});
    return v;
}

// Peers of owner t in the O6 order of sub-slice j (rank offsets j+1 .. n-1, then 1 .. j).
std::vector<uint32_t> O6Peers(uint32_t n, uint32_t t, uint32_t j)
{
    std::vector<uint32_t> v;
    for (uint32_t s = 0; s + 1 < n; ++s) {
        uint32_t x = s + j + 1;
        if (x >= n) x += 1;
        v.push_back((t + x) % n);
    }
    return v;
}

// Emits the folds of one piece [pc.begin, pc.begin + pc.len) of my chunk (chunk-relative coordinates in `subs`):
// own operand at own(e), peer q's at slotOf(q) + (e - pc.begin), result at out(e) — one REDUCE per sub-slice segment.
template <class OwnRef, class OutRef, class SlotRef>
void EmitO6Folds(Builder& b, uint32_t n, uint32_t me, Span pc, const std::vector<Span>& subs, OwnRef own, OutRef out,
                 SlotRef slotOf)
{
    for (uint32_t j = 0; j < subs.size(); ++j) {
        const uint64_t lo = std::max(pc.begin, subs[j].begin);
        const uint64_t hi = std::min(pc.begin + pc.len, subs[j].begin + subs[j].len);
        if (lo >= hi) continue;
        std::vector<Ref> srcs{own(lo)};
        for (uint32_t q : O6Peers(n, me, j)) {
            Ref s = slotOf(q);
            s.off += lo - pc.begin;
            srcs.push_back(s);
        }
        b.Reduce(out(lo), srcs, hi - lo);
    }
}

// AllReduce MeshChunk: executor loops of min(ccl, ccl / 2) (scratch multiple 2, …mesh_chunk.cc:48-55), each sliced
// into n chunks of ceil(count / n) elements (CalcSliceInfoVec :79-97, no 128-B alignment), O6 fold per sub-slice,
// then the mesh all-gather. Pieces of all loops form one pipeline as in the two-shot: step u scatters piece u and
// gathers piece u-2 in one group while piece u-1 is folded.
void AllReduceMeshChunk(const ScheduleParams& p, Builder& b)
{
    const uint32_t n = p.nRanks, me = p.rank;
    const uint64_t loopElems = RefLoopElems(p, p.cclBytes, 2);
    struct Unit {
        uint64_t loopOff, loopCount, t;
    };
    const uint64_t firstChunk = CeilSlice(std::min(loopElems, p.count), n, 0).len;
    // one staging piece per chunk of a loop when it fits (the loop is already the reference's transfer unit)
    const SlotRing slots{0, 2, n - 1, PieceElems(p, 4 * std::max<uint64_t>(1, firstChunk), 2 * (n - 1))};
    const uint64_t pe = slots.pe;
    std::vector<Unit> units;
    for (uint64_t off = 0; off < p.count; off += loopElems) {
        const uint64_t cnt = std::min(loopElems, p.count - off);
        const uint64_t np = NumPieces(CeilSlice(cnt, n, 0).len, pe);
        for (uint64_t t = 0; t < np; ++t) units.push_back({off, cnt, t});
    }
    auto chunk = [&](const Unit& x, uint32_t c) {
        Span s = CeilSlice(x.loopCount, n, c);
        s.begin += x.loopOff;
        return s;
    };
    auto piece = [&](uint64_t u) {
        return [&, u](uint32_t q) { return Piece(chunk(units[u], q), pe, units[u].t); };
    };
    TwoShotPipeline(
        b, units.size(), [&](uint64_t u) { ScatterPieces(b, n, me, piece(u), slots.Peers(u, me)); },
        [&](uint64_t g) { GatherPieces(b, n, me, piece(g)); },
        [&](uint64_t u) {
            const Span mine = chunk(units[u], me);
            const Span pc = Piece({0, mine.len}, pe, units[u].t);  // chunk-relative
            if (pc.len == 0) return;
            EmitO6Folds(b, n, me, pc, SubSlicesEven(mine.len, n - 1),
                        [&](uint64_t e) { return In(mine.begin + e); }, [&](uint64_t e) { return Out(mine.begin + e); },
                        slots.Peers(u, me));
        });
}

// ReduceScatter MeshChunk: executor loops of min(ccl - 1 MiB, (ccl - 1 MiB) / (n-1)) (TMP_MEM_RESERVE_SIZE and
// scratch multiple n-1, ins_v2_reduce_scatter_sole_executor.cc:32,160-175; …meshchunk.cc:66-72) over recvCount,
// each block cut into the 4-KiB-aligned sub-slices, O6 fold per sub-slice.
void ReduceScatterMeshChunk(const ScheduleParams& p, Builder& b)
{
    const uint32_t n = p.nRanks, me = p.rank;
    const uint64_t rc = p.count;
    constexpr uint64_t kReserve = 1ull << 20;
    // the reference has no loop at all when HCCL_BUFFSIZE <= 1 MiB (maxDataCountPerLoop == 0 → HCCL_E_INTERNAL);
    // here the whole CCL size is used then
    const uint64_t tmp = p.cclBytes > kReserve ? p.cclBytes - kReserve : p.cclBytes;
    const uint64_t loopBytes = std::min(tmp, tmp / (n - 1) / kAlignBytes * kAlignBytes);
    const uint64_t loopElems = std::max<uint64_t>(1, loopBytes / p.elemSize);
    const SlotRing slots{0, 2, n - 1, PieceElems(p, std::min(rc, loopElems), 2 * (n - 1))};
    uint64_t u = 0;
    for (uint64_t off = 0; off < rc; off += loopElems) {
        const uint64_t cnt = std::min(loopElems, rc - off);
        const std::vector<Span> subs = SubSlicesRs(cnt, n - 1, p.elemSize);
        const uint64_t np = NumPieces(cnt, slots.pe);
        for (uint64_t t = 0; t < np; ++t, ++u) {
            const Span pc = Piece({0, cnt}, slots.pe, t);  // loop-relative
            const auto slot = slots.Peers(u, me);
            ScatterPieces(b, n, me, [&](uint32_t q) { return Span{uint64_t(q) * rc + off + pc.begin, pc.len}; }, slot);
            b.EndGroup();
            EmitO6Folds(b, n, me, pc, subs, [&](uint64_t e) { return In(uint64_t(me) * rc + off + e); },
                        [&](uint64_t e) { return Out(off + e); }, slot);
        }
    }
}

// ------------------------------------------------------------------------------------------- rings over xGMI
//
// xGMI is point to point: a single directed ring moves every byte over ONE link per rank, 1/7 of what an 8-GPU
// node offers. The ring schedules therefore run R arc-disjoint directed Hamiltonian cycles at once (RingTable):
// the complete digraph on n ranks decomposes into n-1 of them for n != 4, 6 (Tillson), so at n = 8 seven rings use
// all seven outgoing and incoming links of every GPU. The buffer is split into R parts; part k travels around ring
// k. Inside a ring, ranks are addressed by their position v on the cycle (rank = cycle[v]), which is the reference's
// ring neighbour convention prev = v-1, next = v+1 (scatter_ring.cc:186-187) applied to the cycle.

// The rings for n ranks (every rank computes the same table): found by search and checked in tests/test_schedules.py
// (each is a Hamiltonian cycle, no arc is used twice); n > 8: the rotations v -> v + k with gcd(k, n) = 1.
}  // namespace

std::vector<std::vector<uint32_t>> RingTable(uint32_t n)
{
    switch (n) {
        case 1: return {{0}};
        case 2: return {{0, 1}};
        case 3: return {{0, 1, 2}, {0, 2, 1}};
        case 4: return {{0, 1, 3, 2}, {0, 2, 3, 1}};
        case 5: return {{0, 3, 1, 2, 4}, {0, 1, 4, 3, 2}, {0, 4, 2, 1, 3}, {0, 2, 3, 4, 1}};
        case 6: return {{0, 3, 1, 2, 5, 4}, {0, 4, 5, 2, 1, 3}, {0, 2, 3, 4, 1, 5}, {0, 5, 1, 4, 3, 2}};
        case 7:
            return {{0, 5, 1, 6, 4, 3, 2}, {0, 2, 3, 6, 1, 4, 5}, {0, 3, 1, 2, 5, 4, 6}, {0, 4, 1, 5, 2, 6, 3},
                    {0, 1, 3, 5, 6, 2, 4}, {0, 6, 5, 3, 4, 2, 1}};
        case 8:
            return {{0, 5, 6, 3, 7, 2, 1, 4}, {0, 4, 2, 3, 5, 7, 1, 6}, {0, 3, 2, 7, 5, 4, 6, 1},
                    {0, 7, 6, 2, 4, 1, 5, 3}, {0, 2, 6, 5, 1, 3, 4, 7}, {0, 1, 7, 3, 6, 4, 5, 2},
                    {0, 6, 7, 4, 3, 1, 2, 5}};
        default: {
            std::vector<std::vector<uint32_t>> t;
            for (uint32_t k = 1; k < n; ++k) {
                uint32_t a = k, bb = n;
                while (bb != 0) {
                    const uint32_t r = a % bb;
                    a = bb;
                    bb = r;
                }
                if (a != 1) continue;
                std::vector<uint32_t> c;
                for (uint32_t v = 0; v < n; ++v) c.push_back(uint32_t((uint64_t(v) * k) % n));
                t.push_back(c);
            }
            return t;
        }
    }
}

namespace {

// One ring of the table as seen from rank `me`: its cycle and my position on it.
struct RingView {
    std::vector<uint32_t> cyc;
    uint32_t pos;
    uint32_t At(int64_t v) const
    {
        const int64_t n = int64_t(cyc.size());
        return cyc[size_t(((v % n) + n) % n)];
    }
    uint32_t Next() const { return At(int64_t(pos) + 1); }
    uint32_t Prev() const { return At(int64_t(pos) - 1); }
    uint32_t Back(uint32_t d) const { return At(int64_t(pos) - d); }  // the rank d positions behind me
};

// How many of the rings a call uses. Every ring adds two messages per rank and step, about 1 us of host time each on
// the executor (profiles/r02_rccl_selfloop_latency*.jsonl), and spreads the transfer over one more link (1 MiB takes
// 13.65 us at 76.8 GB/s). The AllReduce (2(n-1) steps, 2(n-1)/n x bytes moved), the ReduceScatter and the AllGather
// ((n-1) steps, (n-1)/n x the input / output bytes) all balance at R^2 = 13.65 x MiB / (2n): the largest R with
// R^2 x 2n x 1 MiB <= 13.65 x bytes, at least 1 (one ring up to ~4.7 MiB at n = 8, all seven from ~57 MiB). `bytes` is
// the AllReduce buffer, the ReduceScatter input or the AllGather output of one rank.
std::vector<RingView> Rings(uint32_t n, uint32_t me, uint64_t bytes)
{
    std::vector<std::vector<uint32_t>> table = RingTable(n);
    size_t rings = 1;
    while (rings < table.size() &&
           double(rings + 1) * double(rings + 1) * 2.0 * n * double(1u << 20) <= 13.65 * double(bytes)) {
        ++rings;
    }
    table.resize(std::min(table.size(), rings));
    std::vector<RingView> v;
    for (auto& c : table) {
        RingView r{c, 0};
        for (uint32_t i = 0; i < n; ++i) {
            if (c[i] == me) r.pos = i;
        }
        v.push_back(r);
    }
    return v;
}

// One step on all rings in one group: on ring k, sendOf(k) goes to my next rank and recvOf(k) comes from my previous.
// The parts of a buffer are Chunk(count, R, k, align): ceil(count / R) rounded up to 128 B, trailing parts short or
// empty.
template <class SendOf, class RecvOf>
void RingStep(Builder& b, const std::vector<RingView>& rings, SendOf sendOf, RecvOf recvOf)
{
    for (uint32_t k = 0; k < rings.size(); ++k) {
        const Seg s = sendOf(k), r = recvOf(k);
        b.Send(rings[k].Next(), s.ref, s.len);
        b.Recv(rings[k].Prev(), r.ref, r.len);
    }
    b.EndGroup();
}

// AllReduce over R rings: in part k, position v owns chunk v; n-1 reduce-scatter steps (position v receives chunk
// v-s-2 from v-1 and folds it into its own copy: acc = travelling partial (src) (op) own input), then n-1 all-gather
// steps. Every step posts all rings' transfers in one group; pieces pipeline the steps.
void AllReduceRing(const ScheduleParams& p, Builder& b)
{
    const uint32_t n = p.nRanks, me = p.rank;
    const uint64_t alignElems = AlignElems(p);
    const std::vector<RingView> rings = Rings(n, me, p.count * p.elemSize);
    const uint32_t R = static_cast<uint32_t>(rings.size());
    const Span part0 = Chunk(p.count, R, 0, alignElems);
    const uint64_t maxChunk = Chunk(part0.len, n, 0, alignElems).len;
    const SlotRing slots{0, 4, R, PieceElems(p, maxChunk, 4 * R)};
    const uint64_t pe = slots.pe, np = NumPieces(maxChunk, pe);
    // chunk of ring k at position pos - back (mod n) of its cycle
    auto chunkOf = [&](uint32_t k, uint32_t back) {
        const Span part = Chunk(p.count, R, k, alignElems);
        Span ch = Chunk(part.len, n, (rings[k].pos + 2 * n - back) % n, alignElems);
        ch.begin += part.begin;
        return ch;
    };
    std::vector<Span> rcv(R);
    uint64_t unit = 0;
    for (uint32_t s = 0; s + 1 < n; ++s) {
        for (uint64_t t = 0; t < np; ++t, ++unit) {
            for (uint32_t k = 0; k < R; ++k) rcv[k] = Piece(chunkOf(k, s + 2), pe, t);
            RingStep(
                b, rings,
                [&](uint32_t k) {
                    const Span snd = Piece(chunkOf(k, s + 1), pe, t);
                    return Seg{s == 0 ? In(snd.begin) : Out(snd.begin), snd.len};
                },
                [&](uint32_t k) { return Seg{slots.At(unit, k), rcv[k].len}; });
            for (uint32_t k = 0; k < R; ++k) {
                b.Reduce(Out(rcv[k].begin), {In(rcv[k].begin), slots.At(unit, k)}, rcv[k].len);
            }
        }
    }
    // All-gather: received chunks land in recvBuf directly, so no staging bounds the granule, and there is no fold to
    // pipeline against: every step moves whole chunks on all R rings at once (one transport group per step instead
    // of one per staging piece, which saves a group launch per piece; tools/executor_overlap_model.py).
    for (uint32_t s = 0; s + 1 < n; ++s) {
        RingStep(
            b, rings,
            [&](uint32_t k) {
                const Span snd = chunkOf(k, s);
                return Seg{Out(snd.begin), snd.len};
            },
            [&](uint32_t k) {
                const Span got = chunkOf(k, s + 1);
                return Seg{Out(got.begin), got.len};
            });
    }
}

// Recursive halving (reduce-scatter) then recursive doubling (all-gather), power-of-two n = 2^m
// (docs/zh/user_guide/coll_algo_intro/RHD.md). One RHD instance uses one link per step (partner = rank ^ d), 3 of an
// 8-GPU node's 7. The ranks of a power-of-two world are the vectors of GF(2)^m and the 7 XOR matchings r <-> r ^ v
// (v != 0) partition its links, so the schedule runs up to n-1 instances at once (RhdInstances: fewer for small
// calls), one per part of the buffer: instance j
// relabels ranks by the linear map whose step-s partner vector is alpha^(s+j) in GF(2^m) (alpha primitive). At every
// step the instances' vectors alpha^(s+j), j = 0..n-2, are all the nonzero vectors: every link carries exactly one.
// Inside instance j the classic RHD runs on virtual ranks: region = virtual chunk range [lo, hi); at virtual distance
// d the rank keeps the half selected by bit d of its virtual rank and exchanges the other half with its partner.
// It ends with virtual rank v owning chunk v of the part.

// Multiplication in GF(2^m) modulo a primitive polynomial (m <= 4: x^2+x+1, x^3+x+1, x^4+x+1).
uint32_t Gf2Mul(uint32_t a, uint32_t b, uint32_t m)
{
    static const uint32_t kPoly[5] = {0, 0x3, 0x7, 0xB, 0x13};
    uint32_t r = 0;
    for (uint32_t i = 0; i < m; ++i) {
        if ((b >> i) & 1u) r ^= a << i;
    }
    for (uint32_t i = 2 * m; i-- > m;) {
        if ((r >> i) & 1u) r ^= kPoly[m] << (i - m);
    }
    return r;
}

}  // namespace

std::vector<std::vector<uint32_t>> RhdTable(uint32_t n)
{
    // returns, per instance, virt->real rank (index = virtual rank)
    uint32_t m = 0;
    while ((1u << m) < n) ++m;
    if ((1u << m) != n || m > 4) return {};
    if (m == 0) return {{0}};
    std::vector<std::vector<uint32_t>> t;
    for (uint32_t j = 0; j + 1 < n; ++j) {
        // partner vector of step s (virtual bit m-1-s) is alpha^(s+j), alpha = 2
        std::vector<uint32_t> vec(m);
        for (uint32_t s2 = 0; s2 < m; ++s2) {
            uint32_t x = 1;
            for (uint32_t k = 0; k < s2 + j; ++k) x = Gf2Mul(x, 2, m);
            vec[s2] = x;
        }
        std::vector<uint32_t> real(n);
        for (uint32_t v = 0; v < n; ++v) {
            uint32_t r = 0;
            for (uint32_t s2 = 0; s2 < m; ++s2) {
                if ((v >> (m - 1 - s2)) & 1u) r ^= vec[s2];
            }
            real[v] = r;
        }
        t.push_back(real);
    }
    return t;
}

// How many of the n-1 instances a call of `bytes` per rank runs. Every instance adds one message per rank and step
// (6 steps at n = 8), and on the executor each message costs host time whatever its size: about 10 us per transport
// group plus 1 us per message (RCCL self-loop programs, profiles/r02_rccl_selfloop_latency.jsonl). What an instance
// buys is link bandwidth: R instances spread 2 (n-1)/n x bytes over R links at 76.8 GB/s each. With 12 us per extra
// instance against 22.8 us per MiB / R of transfer, the best R is about sqrt(2 x bytes / 1 MiB): one instance up to
// 1 MiB (C5's latency range), all seven from 24.5 MiB. Ranks agree: it depends on the call's arguments only.
uint32_t RhdInstances(uint32_t n, uint64_t bytes)
{
    const uint32_t most = n > 1 ? n - 1 : 1;
    uint32_t r = 1;
    while (r < most && uint64_t(r + 1) * (r + 1) * (1ull << 20) <= 2 * bytes) ++r;
    return r;
}

namespace {

void AllReduceRhd(const ScheduleParams& p, Builder& b)
{
    const uint32_t n = p.nRanks, me = p.rank;
    const uint64_t alignElems = AlignElems(p);
    std::vector<std::vector<uint32_t>> table = RhdTable(n);
    table.resize(std::min<size_t>(table.size(), RhdInstances(n, p.count * p.elemSize)));
    const uint32_t R = static_cast<uint32_t>(table.size());
    struct Inst {
        std::vector<uint32_t> real;
        uint32_t v;  // my virtual rank
        Span part;
        uint32_t lo, hi;
    };
    std::vector<Inst> inst(R);
    for (uint32_t j = 0; j < R; ++j) {
        inst[j].real = table[j];
        for (uint32_t v = 0; v < n; ++v) {
            if (table[j][v] == me) inst[j].v = v;
        }
        inst[j].part = Chunk(p.count, R, j, alignElems);
        inst[j].lo = 0;
        inst[j].hi = n;
    }
    auto range = [&](const Inst& I, uint32_t lo, uint32_t hi) {
        Span a = Chunk(I.part.len, n, lo, alignElems);
        Span z = Chunk(I.part.len, n, hi - 1, alignElems);
        return Span{I.part.begin + a.begin, z.begin + z.len - a.begin};
    };
    const SlotRing slots{0, 4, R, PieceElems(p, range(inst[0], 0, n / 2).len, 4 * R)};
    const uint64_t pe = slots.pe;
    uint64_t unit = 0;
    bool first = true;
    for (uint32_t d = n / 2; d >= 1; d /= 2) {
        // the piece count is the same on every rank (partners of different instances share groups): the widest
        // half any rank can hold at this distance is the first d chunks of part 0
        const uint64_t np = NumPieces(range(inst[0], 0, d).len, pe);
        std::vector<Span> keep(R), give(R);
        for (uint32_t j = 0; j < R; ++j) {
            const Inst& I = inst[j];
            const uint32_t mid = I.lo + d;
            const bool keepLow = (I.v & d) == 0;
            keep[j] = keepLow ? range(I, I.lo, mid) : range(I, mid, I.hi);
            give[j] = keepLow ? range(I, mid, I.hi) : range(I, I.lo, mid);
        }
        for (uint64_t t = 0; t < np; ++t, ++unit) {
            for (uint32_t j = 0; j < R; ++j) {
                const uint32_t partner = inst[j].real[inst[j].v ^ d];
                const Span g = Piece(give[j], pe, t);
                const Span k = Piece(keep[j], pe, t);
                b.Send(partner, first ? In(g.begin) : Out(g.begin), g.len);
                b.Recv(partner, slots.At(unit, j), k.len);
            }
            b.EndGroup();
            for (uint32_t j = 0; j < R; ++j) {
                const Span k = Piece(keep[j], pe, t);
                b.Reduce(Out(k.begin), {first ? In(k.begin) : Out(k.begin), slots.At(unit, j)}, k.len);
            }
        }
        for (Inst& I : inst) {
            const uint32_t mid = I.lo + d;
            if ((I.v & d) == 0) {
                I.hi = mid;
            } else {
                I.lo = mid;
            }
        }
        first = false;
        if (d == 1) break;
    }
    // Recursive doubling: the exchanged halves land in recvBuf directly (no staging, no fold), so every step moves
    // whole regions in one transport group (as the ring's all-gather).
    for (uint32_t d = 1; d < n; d *= 2) {
        std::vector<Span> mine(R), theirs(R);
        std::vector<uint32_t> plo(R);
        for (uint32_t j = 0; j < R; ++j) {
            const Inst& I = inst[j];
            // my region is [lo, lo + d) virtual chunks; the partner's is the adjacent block of d chunks
            plo[j] = (I.v & d) == 0 ? I.lo + d : I.lo - d;
            mine[j] = range(I, I.lo, I.lo + d);
            theirs[j] = range(I, plo[j], plo[j] + d);
        }
        for (uint32_t j = 0; j < R; ++j) {
            const uint32_t partner = inst[j].real[inst[j].v ^ d];
            b.Send(partner, Out(mine[j].begin), mine[j].len);
            b.Recv(partner, Out(theirs[j].begin), theirs[j].len);
        }
        b.EndGroup();
        for (uint32_t j = 0; j < R; ++j) inst[j].lo = std::min(inst[j].lo, plo[j]);
    }
}

// NHR (ins_temp_all_reduce_nhr.cc:171-173, 230-369, 390-482): ceil(log2 n) reduce-scatter steps in which rank r
// sends slices r-2^k, r-2^k-2^(k+1), ... to r-2^k and receives slices r, r-2^(k+1), ... from r+2^k, folding each as
// receiver partial (dst) (op) sender partial (src); then the mirrored all-gather. Slices are floor(count/n) with the
// tail on the last slice. The reference works in its CCL buffer (PreCopy / PostCopy); here recvBuf is the working
// buffer, which gives the same per-element order.
struct NhrStep {
    uint32_t to, from;
    std::vector<uint32_t> tx, rx;
};

std::vector<NhrStep> NhrSteps(uint32_t n, uint32_t me, bool gather)
{
    uint32_t nSteps = 0;
    for (uint32_t t = n - 1; t != 0; t >>= 1) nSteps++;
    std::vector<NhrStep> out(nSteps);
    for (uint32_t step = 0; step < nSteps; ++step) {
        NhrStep& st = out[step];
        uint32_t nSlices, delta, tx, rx;
        if (!gather) {
            const uint32_t dr = 1u << step;
            st.to = (me + n - dr) % n;
            st.from = (me + dr) % n;
            nSlices = (n - 1 + (1u << step)) / (1u << (step + 1));
            delta = 1u << (step + 1);
            tx = st.to;
            rx = me;
        } else {
            const uint32_t dr = 1u << (nSteps - 1 - step);
            st.to = (me + dr) % n;
            st.from = (me + n - dr) % n;
            nSlices = (n - 1 + dr) / (1u << (nSteps - step));
            delta = 1u << (nSteps - step);
            tx = me;
            rx = (me + n - dr) % n;
        }
        for (uint32_t i = 0; i < nSlices; ++i) {
            st.tx.push_back(tx);
            st.rx.push_back(rx);
            tx = (tx + n - delta % n) % n;
            rx = (rx + n - delta % n) % n;
        }
    }
    return out;
}

// The staging slots of the NHR steps, one per slice a step can receive ((n+1)/2 at most), behind a working area of
// `workElems` staging elements; the working area comes off the capacity that bounds the pieces.
SlotRing NhrSlots(const ScheduleParams& p, uint64_t workElems, uint64_t widest)
{
    const uint64_t maxSlices = (p.nRanks + 1) / 2;
    ScheduleParams pp = p;
    if (pp.scratchCapBytes != 0) pp.scratchCapBytes -= std::min(pp.scratchCapBytes, workElems * p.elemSize);
    return {workElems, 2, maxSlices, PieceElems(pp, widest, 2 * maxSlices)};
}

// The NHR steps on a working buffer: slice(i) is slice i in the coordinates of work(off), `widest` the longest slice
// (every rank cuts the same pieces). A reduce-scatter step sends the tx slices, receives the rx slices into `slots`,
// ends the group and folds each as receiver partial (dst) (op) sender partial (src); the all-gather phase (`gather`)
// receives in place.
template <class SliceOf, class WorkRef>
void NhrRun(Builder& b, uint32_t n, uint32_t me, SliceOf slice, WorkRef work, const SlotRing& slots, uint64_t widest,
            bool gather)
{
    const uint64_t pe = slots.pe, np = NumPieces(widest, pe);
    uint64_t unit = 0;
    for (int phase = 0; phase < (gather ? 2 : 1); ++phase) {
        const bool ag = phase == 1;
        for (const NhrStep& st : NhrSteps(n, me, ag)) {
            for (uint64_t t = 0; t < np; ++t, ++unit) {
                for (size_t i = 0; i < st.tx.size(); ++i) {
                    const Span s = Piece(slice(st.tx[i]), pe, t);
                    b.Send(st.to, work(s.begin), s.len);
                }
                for (size_t i = 0; i < st.rx.size(); ++i) {
                    const Span s = Piece(slice(st.rx[i]), pe, t);
                    b.Recv(st.from, ag ? work(s.begin) : slots.At(unit, i), s.len);
                }
                b.EndGroup();
                if (ag) continue;
                for (size_t i = 0; i < st.rx.size(); ++i) {
                    const Span s = Piece(slice(st.rx[i]), pe, t);
                    b.Reduce(work(s.begin), {work(s.begin), slots.At(unit, i)}, s.len);
                }
            }
        }
    }
}

void AllReduceNhrLoop(const ScheduleParams& p, Builder& b)
{
    const uint32_t n = p.nRanks;
    auto slice = [&](uint32_t i) { return FloorSlice(p.count, n, i); };
    const uint64_t tail = slice(n - 1).len;
    b.Copy(Out(0), In(0), p.count);  // PreCopy (ins_temp_all_reduce_nhr.cc PreCopy): the working buffer
    NhrRun(b, n, p.rank, slice, Out, NhrSlots(p, 0, tail), tail, true);
}

void AllReduceNhr(const ScheduleParams& p, Builder& b)
{
    ForEachRefLoop(p, b, RefLoopElems(p, p.cclBytes, 1), [&](const ScheduleParams& lp) { AllReduceNhrLoop(lp, b); });
}

// NHR ReduceScatter (ins_temp_reduce_scatter_nhr.cc:104-197, 278-397, 407-456): the NHR reduce-scatter steps with the
// ReduceScatter blocks as slices (block i = slice i, whatever the executor loop, so the order does not depend on the
// loop size), write-reduce receiver partial (dst) (op) sender partial (src), then block `me` to recvBuf. Blocks are
// processed in columns of W elements: n working columns in the first ccl bytes of staging, receive slots after them.
void ReduceScatterNhr(const ScheduleParams& p, Builder& b)
{
    const uint32_t n = p.nRanks, me = p.rank;
    const uint64_t rc = p.count;
    const uint64_t alignElems = AlignElems(p);
    const uint64_t W = std::min(rc, std::max(alignElems, p.cclBytes / n / p.elemSize / alignElems * alignElems));
    for (uint64_t col = 0; col < rc; col += W) {
        const uint64_t w = std::min(W, rc - col);
        auto column = [&](uint32_t i) { return Span{uint64_t(i) * W, w}; };  // working column i, in staging
        for (uint32_t i = 0; i < n; ++i) b.Copy(Scr(column(i).begin), In(uint64_t(i) * rc + col), w);  // LocalDataCopy
        NhrRun(b, n, me, column, Scr, NhrSlots(p, n * W, w), w, false);
        b.Copy(Out(col), Scr(column(me).begin), w);  // PostLocalCopy
    }
}

// ------------------------------------------------------------------------------------------- STRICT tree (O4)

// Order-preserved tree fold. At n <= 8 (MAX_RANK_NUM_FOR_ORDER_PRESERVED, order_preserved_common.h:22), which is every
// single-node case, the reference selects AicpuReduceScatterStrictOrderedMesh / AicpuAllReduceStrictOrderedMesh
// (reduce_scatter_auto_selector.cc:406-413, all_reduce_auto_selector.cc:412-418), i.e. the template
// InsTempReduceScatterOrderPreservedLevel1: its all-to-all puts source s's block for receiver t into t's CCL slot
// CalcOutputIndex(t, s) = (t + s) % n (…order_preserved_level1.cc:176-181, 274-278; own block :196-215), and its
// RunLocalReduce reads virtual index v from slot CalcOutputIndex(v, t) (:322-400), so virtual index = source rank on
// every receiver (tests/test_strict_level1.py restates the template and checks it against this schedule). Above 8
// ranks the Group template folds the same tree (ins_temp_reduce_scatter_order_preserved_group.cc:305-399). The tree:
// while more than one block remains, M = largest power of two below the count and block i >= M is folded into block
// i % M as dst = src (op) dst. n = 8: ((x0+x4)+(x2+x6))+((x1+x5)+(x3+x7)). Rank-independent.
// `blocks` must be writable (staging); the last fold writes `out`.
void EmitTree(Builder& b, const std::vector<Ref>& blocks, Ref out, uint64_t count)
{
    uint32_t remaining = static_cast<uint32_t>(blocks.size());
    if (remaining == 1) {
        b.Copy(out, blocks[0], count);
        return;
    }
    while (remaining > 1) {
        uint32_t m = 1;
        while (m * 2 < remaining) m *= 2;
        for (uint32_t src = m; src < remaining; ++src) {
            const uint32_t dst = src % m;
            b.Reduce(m == 1 ? out : blocks[dst], {blocks[dst], blocks[src]}, count);
        }
        remaining = m;
    }
}

// The tree over per-source staging slots slotOf(0..n-1): the own block is copied into its slot first (as PreLocalCopy
// does, …order_preserved_level1.cc:215-232), the peers' are already there.
template <class SlotOf>
void TreeFold(Builder& b, uint32_t n, uint32_t me, Ref own, Ref out, uint64_t count, SlotOf slotOf)
{
    b.Copy(slotOf(me), own, count);
    std::vector<Ref> blocks;
    for (uint32_t q = 0; q < n; ++q) blocks.push_back(slotOf(q));
    EmitTree(b, blocks, out, count);
}

// ReduceScatter in STRICT order: mesh exchange of blocks into per-source staging slots (own block copied in, as
// PreLocalCopy does, :215-232), then the tree fold into recvBuf.
void ReduceScatterTree(const ScheduleParams& p, Builder& b)
{
    const uint32_t n = p.nRanks, me = p.rank;
    const uint64_t rc = p.count;
    const SlotRing slots{0, 2, n, PieceElems(p, rc, 2 * n)};
    const uint64_t np = NumPieces(rc, slots.pe);
    for (uint64_t t = 0; t < np; ++t) {
        const Span s = Piece({0, rc}, slots.pe, t);
        auto block = [&](uint32_t q) { return Span{uint64_t(q) * rc + s.begin, s.len}; };  // piece t of input block q
        auto slot = [&](uint32_t q) { return slots.At(t, q); };
        ScatterPieces(b, n, me, block, slot);
        b.EndGroup();
        TreeFold(b, n, me, In(block(me).begin), Out(s.begin), s.len, slot);
    }
}

// AllReduce in STRICT order: the two-shot structure with a slot per rank and the tree fold in place of the O2 chain.
void AllReduceTree(const ScheduleParams& p, Builder& b)
{
    const uint32_t n = p.nRanks, me = p.rank;
    AllReduceTwoShotWith(p, b, true, [&](Span rs, auto slotOf) {
        TreeFold(b, n, me, In(rs.begin), Out(rs.begin), rs.len, slotOf);
    });
}

// ------------------------------------------------------------------------------------------- ReduceScatter

// Mesh (O1): every rank sends block q to rank q; rank me folds its own block first, then peers ascending
// (ins_temp_reduce_scatter_mesh_1D.cc:138-206). count = recvCount, input block q at q * count.
void ReduceScatterMesh(const ScheduleParams& p, Builder& b)
{
    const uint32_t n = p.nRanks, me = p.rank;
    const uint64_t rc = p.count;
    const SlotRing slots{0, 2, n - 1, PieceElems(p, rc, 2 * (n - 1))};
    const uint64_t np = NumPieces(rc, slots.pe);
    for (uint64_t t = 0; t < np; ++t) {
        const Span s = Piece({0, rc}, slots.pe, t);
        auto block = [&](uint32_t q) { return Span{uint64_t(q) * rc + s.begin, s.len}; };  // piece t of input block q
        const auto slot = slots.Peers(t, me);
        ScatterPieces(b, n, me, block, slot);
        b.EndGroup();
        b.Reduce(Out(s.begin), O1Srcs(In(block(me).begin), n, me, slot), s.len);
    }
}

// ReduceScatterV mesh (O1, ins_temp_reduce_scatter_v_mesh_1D.cc:107-146, RunReduceScatterV :148-205): every rank
// writes its input block of peer q, [displs[q], displs[q] + counts[q]), to q; rank me copies its own block to recvBuf
// and folds the peers' copies into it in ascending rank order (PostCopy's LocalReduce loop over tmpRank). Pieces of
// counts[me] are pipelined through two staging slot sets as in the mesh ReduceScatter; the order does not depend on
// them.
void ReduceScatterVMesh(const ScheduleParams& p, Builder& b)
{
    const uint32_t n = p.nRanks, me = p.rank;
    uint64_t widest = 0;
    for (uint32_t q = 0; q < n; ++q) widest = std::max(widest, p.counts[q]);
    const SlotRing slots{0, 2, n - 1, PieceElems(p, std::max<uint64_t>(1, widest), 2 * (n - 1))};
    const uint64_t np = NumPieces(widest, slots.pe);  // equal on every rank
    for (uint64_t t = 0; t < np; ++t) {
        // piece t of rank q's block, in input coordinates
        auto piece = [&](uint32_t q) { return Piece({p.displs[q], p.counts[q]}, slots.pe, t); };
        const auto slot = slots.Peers(t, me);
        ScatterPieces(b, n, me, piece, slot);
        b.EndGroup();
        const Span mine = piece(me);
        if (mine.len == 0) continue;
        b.Reduce(Out(mine.begin - p.displs[me]), O1Srcs(In(mine.begin), n, me, slot), mine.len);
    }
}

// Ring reduce-scatter over R rings: every block is split into R parts and part k of every block travels around ring
// k. Step s, position v sends block cycle[v-s-1] (its partial) to v+1 and folds block cycle[v-s-2] received from v-1
// into its own input (acc = travelling partial (src) (op) own input); position v ends with block cycle[v] = its own.
// Partials live in staging until forwarded, the last step writes recvBuf. Rounds of kRound pieces bound the staging.
void ReduceScatterRing(const ScheduleParams& p, Builder& b)
{
    const uint32_t n = p.nRanks, me = p.rank;
    const uint64_t rc = p.count;
    const uint64_t alignElems = AlignElems(p);
    const std::vector<RingView> rings = Rings(n, me, rc * n * p.elemSize);
    const uint32_t R = static_cast<uint32_t>(rings.size());
    const uint64_t kRound = 4;
    const uint64_t maxPart = Chunk(rc, R, 0, alignElems).len;
    // two slot sets by step parity (step s receives into set s % 2 what step s+1 forwards), each one slot per ring and
    // piece of the round
    const SlotRing slots{0, 2, R * kRound, PieceElems(p, maxPart, 2 * kRound * R)};
    const uint64_t pe = slots.pe, np = NumPieces(maxPart, pe);
    std::vector<Span> piece(R);
    for (uint64_t r0 = 0; r0 < np; r0 += kRound) {
        const uint64_t r1 = std::min(np, r0 + kRound);
        for (uint32_t s = 0; s + 1 < n; ++s) {
            for (uint64_t t = r0; t < r1; ++t) {
                for (uint32_t k = 0; k < R; ++k) piece[k] = Piece(Chunk(rc, R, k, alignElems), pe, t);
                auto slot = [&](uint32_t step, uint32_t k) { return slots.At(step, k * kRound + (t - r0)); };
                // my input of the block `back` positions behind me on ring k
                auto own = [&](uint32_t k, uint32_t back) { return In(uint64_t(rings[k].Back(back)) * rc + piece[k].begin); };
                RingStep(
                    b, rings, [&](uint32_t k) { return Seg{s == 0 ? own(k, s + 1) : slot(s + 1, k), piece[k].len}; },
                    [&](uint32_t k) { return Seg{slot(s, k), piece[k].len}; });
                for (uint32_t k = 0; k < R; ++k) {
                    b.Reduce((s + 2 == n) ? Out(piece[k].begin) : slot(s, k), {own(k, s + 2), slot(s, k)}, piece[k].len);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------- Reduce

// Mesh one-shot (O1, me = root): peers send their whole input to the root, which folds own + peers ascending
// (reduce_mesh_1D.cc:136-249). Non-root recvBuf is not touched.
void ReduceOneShot(const ScheduleParams& p, Builder& b)
{
    const uint32_t n = p.nRanks, me = p.rank, root = p.root;
    const SlotRing slots{0, 2, n - 1, PieceElems(p, p.count, 2 * (n - 1))};
    const uint64_t np = CeilDiv(p.count, slots.pe);
    for (uint64_t t = 0; t < np; ++t) {
        const Span s = Piece({0, p.count}, slots.pe, t);
        if (me != root) {
            b.Send(root, In(s.begin), s.len);
            b.EndGroup();
            continue;
        }
        const auto slot = slots.Peers(t, root);
        for (uint32_t q : PeerOrder(n, me)) b.Recv(q, slot(q), s.len);  // one direction: the root only receives
        b.EndGroup();
        b.Reduce(Out(s.begin), O1Srcs(In(s.begin), n, me, slot), s.len);
    }
}

// Two-shot: mesh reduce-scatter with O1 per chunk owner (reduce_mesh_1D_two_shot.cc:209-249), then the owners send
// their reduced chunks to the root. Non-roots fold into a staging slot, so their recvBuf is not touched. Slices are
// the template's balanced split of each executor loop (scratch multiple n, transport bound UB_MAX_DATA_SIZE).
void ReduceTwoShotLoop(const ScheduleParams& p, Builder& b)
{
    const uint32_t n = p.nRanks, me = p.rank, root = p.root;
    const uint64_t maxChunk = BalancedSlice(p.count, n, 0).len;
    // slots: 2 x (n-1) receive pieces + 2 reduced pieces (non-root)
    const uint64_t pe = PieceElems(p, maxChunk, 2 * n);
    const SlotRing slots{0, 2, n - 1, pe}, red{2 * (n - 1) * pe, 2, 1, pe};
    auto piece = [&](uint64_t t) {
        return [&p, n, pe, t](uint32_t q) { return Piece(BalancedSlice(p.count, n, q), pe, t); };
    };
    TwoShotPipeline(
        b, NumPieces(maxChunk, pe), [&](uint64_t t) { ScatterPieces(b, n, me, piece(t), slots.Peers(t, me)); },
        [&](uint64_t g) {
            // one direction: the owners' reduced pieces go to the root
            if (me == root) {
                for (uint32_t q : PeerOrder(n, me)) {
                    const Span theirs = piece(g)(q);
                    b.Recv(q, Out(theirs.begin), theirs.len);
                }
            } else {
                b.Send(root, red.At(g, 0), piece(g)(me).len);
            }
        },
        [&](uint64_t t) {
            const Span rs = piece(t)(me);
            b.Reduce(me == root ? Out(rs.begin) : red.At(t, 0), O1Srcs(In(rs.begin), n, me, slots.Peers(t, me)),
                     rs.len);
        });
}

void ReduceTwoShot(const ScheduleParams& p, Builder& b)
{
    ForEachRefLoop(p, b, RefLoopElems(p, kUbMaxDataSize, p.nRanks),
                   [&](const ScheduleParams& lp) { ReduceTwoShotLoop(lp, b); });
}

// NHR Reduce (reduce_nhr.cc:56-106, 164-267, 294-368): the NHR reduce-scatter and all-gather steps over ceil-sized
// slices of each executor loop (scratch multiple 1, transport bound UB_MAX_DATA_SIZE); only the root keeps the result
// (PostCopy :269-292). The working buffer is recvBuf on the root and staging elsewhere (a non-root recvBuf is never
// written); receive slots follow it in staging.
void ReduceNhrLoop(const ScheduleParams& p, Builder& b)
{
    const uint32_t n = p.nRanks;
    const bool isRoot = p.rank == p.root;
    auto slice = [&](uint32_t i) { return CeilSlice(p.count, n, i); };
    // every rank reserves the working area in its staging (the root does not use it), so that all ranks cut the
    // same pieces
    const uint64_t workElems = AlignUp(p.count, AlignElems(p));
    auto work = [&](uint64_t off) { return isRoot ? Out(off) : Scr(off); };
    const uint64_t widest = slice(0).len;
    b.Copy(work(0), In(0), p.count);  // PreCopy (reduce_nhr.cc:140-162)
    NhrRun(b, n, p.rank, slice, work, NhrSlots(p, workElems, widest), widest, true);
}

void ReduceNhr(const ScheduleParams& p, Builder& b)
{
    ForEachRefLoop(p, b, RefLoopElems(p, kUbMaxDataSize, 1), [&](const ScheduleParams& lp) { ReduceNhrLoop(lp, b); });
}

// ------------------------------------------------------------------------------------------- AllGather

// Mesh: own block copied locally, every piece of the input sent to every peer in one group
// (the all-gather half of ins_temp_all_reduce_mesh_1D_two_shot.cc:340-432 as an operator).
void AllGatherMesh(const ScheduleParams& p, Builder& b)
{
    const uint32_t n = p.nRanks, me = p.rank;
    const uint64_t sc = p.count;
    const uint64_t pe = PieceElems(p, sc, 0);
    const uint64_t np = NumPieces(sc, pe);
    b.Copy(Out(uint64_t(me) * sc), In(0), sc);
    for (uint64_t t = 0; t < np; ++t) {
        const Span s = Piece({0, sc}, pe, t);
        MeshExchange(
            b, n, me, [&](uint32_t) { return Seg{In(s.begin), s.len}; },
            [&](uint32_t q) { return Seg{Out(uint64_t(q) * sc + s.begin), s.len}; });
        b.EndGroup();
    }
}

// All-gather over R rings: part k of every block travels around ring k; step s forwards block cycle[v-s] to v+1 and
// receives block cycle[v-s-1] from v-1.
void AllGatherRing(const ScheduleParams& p, Builder& b)
{
    const uint32_t n = p.nRanks, me = p.rank;
    const uint64_t sc = p.count;
    const uint64_t alignElems = AlignElems(p);
    const std::vector<RingView> rings = Rings(n, me, sc * n * p.elemSize);
    const uint32_t R = static_cast<uint32_t>(rings.size());
    const uint64_t maxPart = Chunk(sc, R, 0, alignElems).len;
    const uint64_t pe = PieceElems(p, maxPart, 0);
    const uint64_t np = NumPieces(maxPart, pe);
    b.Copy(Out(uint64_t(me) * sc), In(0), sc);
    std::vector<Span> piece(R);
    for (uint32_t s = 0; s + 1 < n; ++s) {
        for (uint64_t t = 0; t < np; ++t) {
            for (uint32_t k = 0; k < R; ++k) piece[k] = Piece(Chunk(sc, R, k, alignElems), pe, t);
            // block at `back` positions behind me on ring k, piece t of its part k
            auto block = [&](uint32_t k, uint32_t back) { return Out(uint64_t(rings[k].Back(back)) * sc + piece[k].begin); };
            RingStep(
                b, rings, [&](uint32_t k) { return Seg{s == 0 ? In(piece[k].begin) : block(k, s), piece[k].len}; },
                [&](uint32_t k) { return Seg{block(k, s + 1), piece[k].len}; });
        }
    }
}

// ------------------------------------------------------------------------------------------- Broadcast

// Mesh two-shot (ins_temp_broadcast_mesh_1D_two_shot.cc:69-97, 136-260): n chunks of ceil(count / n) elements. Scatter:
// the root sends rank c chunk c and its own chunk. Gather: the other ranks exchange their chunks among themselves.
// The buffer is the user's one (INPUT = OUTPUT), nothing is staged or folded. Pieces are pipelined: one group holds the
// scatter of piece u and the gather of piece u - 1, which touch different pieces of the buffer.
void BroadcastTwoShot(const ScheduleParams& p, Builder& b)
{
    const uint32_t n = p.nRanks, me = p.rank, root = p.root;
    const uint64_t maxChunk = CeilSlice(p.count, n, 0).len;
    // Default granule: the whole chunk, up to 16 MiB. There is no fold to hide behind a transfer, so a piece only buys
    // the overlap of one piece's scatter with the previous one's gather, and costs a transport group; the quarter-slice
    // default of the reducing schedules cut a 2 MiB chunk (16 MiB on 8 ranks) into four pieces and posted five groups
    // where the AllGather posts four. One piece makes two groups, whatever the payload below 16 MiB x n.
    ScheduleParams gp = p;
    if (gp.pieceBytes == 0) gp.pieceBytes = std::clamp<uint64_t>(maxChunk * p.elemSize, 256ull << 10, 16ull << 20);
    const uint64_t pe = PieceElems(gp, maxChunk, 0);
    const uint64_t np = NumPieces(maxChunk, pe);
    auto piece = [&](uint32_t q, uint64_t t) { return Piece(CeilSlice(p.count, n, q), pe, t); };
    for (uint64_t u = 0; u < np + 1; ++u) {
        if (u < np) {
            const Span rootPiece = piece(root, u);
            if (me == root) {
                for (uint32_t q : PeerOrder(n, me)) {
                    const Span theirs = piece(q, u);
                    b.Send(q, In(theirs.begin), theirs.len);
                    b.Send(q, In(rootPiece.begin), rootPiece.len);
                }
            } else {
                const Span mine = piece(me, u);
                b.Recv(root, Out(mine.begin), mine.len);
                b.Recv(root, Out(rootPiece.begin), rootPiece.len);
            }
        }
        if (u >= 1 && me != root) {
            const Span mine = piece(me, u - 1);
            for (uint32_t q : PeerOrder(n, me)) {
                if (q == root) continue;
                const Span theirs = piece(q, u - 1);
                b.Send(q, Out(mine.begin), mine.len);
                b.Recv(q, Out(theirs.begin), theirs.len);
            }
        }
        b.EndGroup();
    }
}

// ------------------------------------------------------------------------------------------- All-to-all

// Mesh (ins_temp_all_to_all_v_mesh_1D.cc, the reference's only single-node AICPU shape): the own block is copied, and
// every peer q is sent counts[q] elements at displs[q] of the input and received from, recvCounts[q] elements at
// recvDispls[q] of the output. Nothing is staged or folded. Zero counts post nothing; both ends of a pair hold the same
// count, so the programs still match. Default granule: one transport group for the whole call (there is no fold to
// overlap, and a group costs about 10 us of host time). An explicit pieceBytes cuts every pair's message by piece index:
// group u holds piece u of every pair that has one, so ranks may post different numbers of groups; a pair's pieces
// sit in groups of the same index on both ends and no rank skips an index, which keeps the groups live under RCCL's
// rendezvous (tests/test_alltoall_schedule.py).
// The per-peer loop the mesh data-movement operators share: sc / sd and rc / rd are this rank's send and receive counts
// and displacements (n entries each), as the all-to-all takes them. postCopy puts the own-block COPY behind the groups
// instead of ahead of them.
using Counts = std::vector<uint64_t>;
void MeshBlocks(const ScheduleParams& p, Builder& b, const Counts& sc, const Counts& sd, const Counts& rc,
                const Counts& rd, bool postCopy)
{
    const uint32_t n = p.nRanks, me = p.rank;
    if (!postCopy) b.Copy(Out(rd[me]), In(sd[me]), sc[me]);
    uint64_t widest = 0;
    for (uint32_t q = 0; q < n; ++q) {
        if (q != me) widest = std::max({widest, sc[q], rc[q]});
    }
    const uint64_t alignElems = AlignElems(p);
    const uint64_t pe = p.pieceBytes == 0
                            ? std::max<uint64_t>(widest, 1)
                            : std::max<uint64_t>(alignElems, p.pieceBytes / p.elemSize / alignElems * alignElems);
    for (uint64_t u = 0; u * pe < widest; ++u) {
        MeshExchange(
            b, n, me,
            [&](uint32_t q) {
                const Span s = Piece({sd[q], sc[q]}, pe, u);
                return Seg{In(s.begin), s.len};
            },
            [&](uint32_t q) {
                const Span r = Piece({rd[q], rc[q]}, pe, u);
                return Seg{Out(r.begin), r.len};
            });
        b.EndGroup();
    }
    if (postCopy) b.Copy(Out(rd[me]), In(sd[me]), sc[me]);
}

void AllToAllMesh(const ScheduleParams& p, Builder& b)
{
    MeshBlocks(p, b, p.counts, p.displs, p.recvCounts, p.recvDispls, false);
}

// ------------------------------------------------------------------------------------------- Scatter, AllGatherV

// Scatter, mesh (ins_temp_scatter_mesh_1D.cc): the root sends block q of its input to rank q, which receives it at the
// head of its output; the root's own block is copied. The all-to-all's loop with the root's row as the only non-zero
// one. The COPY comes last, as the reference's PostCopy does (:182-214): with recvBuf == sendBuf on a root other than
// 0 it writes where block 0's SEND reads, so it must follow that SEND in program order (the single-stream executor)
// and the two ranges conflict (PlanUnits makes the copy wait for the group; tests/test_scatter_gatherv_schedule.py).
void ScatterMesh(const ScheduleParams& p, Builder& b)
{
    const uint32_t n = p.nRanks, me = p.rank, root = p.root;
    Counts sc(n, 0), sd(n, 0), rc(n, 0), rd(n, 0);
    rc[root] = p.count;
    if (me == root) {
        for (uint32_t q = 0; q < n; ++q) {
            sc[q] = p.count;
            sd[q] = uint64_t(q) * p.count;
        }
    }
    MeshBlocks(p, b, sc, sd, rc, rd, true);
}

// AllGatherV, mesh (ins_temp_all_gather_v_mesh_1D.cc): counts / displs are every rank's block of the output, equal on
// all ranks. The all-to-all's loop where every peer is sent the whole input; the own block's COPY is skipped in place
// (the input is that block of the output).
void AllGatherVMesh(const ScheduleParams& p, Builder& b)
{
    const uint32_t n = p.nRanks, me = p.rank;
    Counts sc(n, p.counts[me]), sd(n, 0);
    if (p.inPlace) sc[me] = 0;
    MeshBlocks(p, b, sc, sd, p.counts, p.displs, false);
}

// ------------------------------------------------------------------------------------------- Barrier

// The barrier moves no user data: every record carries a token of one element. Send k of the program reads element k
// of INPUT and receive k writes element k of OUTPUT, so no two records of a group (nor of the program) share a byte.
// The operator passes the communicator's token allocation as both buffers (Comm::barrierTokens); nothing is staged.

// NHR (RunNHRBarrier, ins_temp_barrier_nhr_aicpu.cc:69-140): nSteps = ceil(log2 n) steps; in step s, with
// delta = 1 << (nSteps - 1 - s), the rank sends a token to (rank + delta) % n and receives one from
// (rank - delta + n) % n. After the steps every rank has heard, directly or through others, from every rank: the
// deltas are the binary digits of every distance 0 .. n - 1. The reference orders each step's send and receive by the
// two peers' ranks so that its blocking writes cannot wait for each other; one transport group per step posts both at
// once (RCCL's group), which makes that ordering unnecessary.
void BarrierNhr(const ScheduleParams& p, Builder& b)
{
    const uint32_t n = p.nRanks, me = p.rank;
    uint32_t nSteps = 0;
    while ((1u << nSteps) < n) ++nSteps;
    for (uint32_t s = 0; s < nSteps; ++s) {
        const uint32_t delta = 1u << (nSteps - 1 - s);
        b.Send((me + delta) % n, In(s), 1);
        b.Recv((me + n - delta) % n, Out(s), 1);
        b.EndGroup();
    }
}

// Mesh1D (RunBarrierMesh, ins_temp_barrier_mesh_1D.cc:79-111): one group with a token to and from every peer.
void BarrierMesh(const ScheduleParams& p, Builder& b)
{
    const uint32_t n = p.nRanks, me = p.rank;
    MeshExchange(
        b, n, me, [&](uint32_t q) { return Seg{In(PeerSlot(q, me)), 1}; },
        [&](uint32_t q) { return Seg{Out(PeerSlot(q, me)), 1}; });
    b.EndGroup();
}

bool IsPow2(uint32_t n) { return n != 0 && (n & (n - 1)) == 0; }

using Generator = void (*)(const ScheduleParams&, Builder&);
struct GeneratorEntry {
    int32_t opType, algo;
    Generator gen;
};
constexpr GeneratorEntry kGenerators[] = {
    {HCCL_AMD_OP_ALLREDUCE, HCCL_AMD_ALGO_MESH_ONESHOT, AllReduceOneShot},
    {HCCL_AMD_OP_ALLREDUCE, HCCL_AMD_ALGO_MESH_TWOSHOT, AllReduceTwoShot},
    {HCCL_AMD_OP_ALLREDUCE, HCCL_AMD_ALGO_RING, AllReduceRing},
    {HCCL_AMD_OP_ALLREDUCE, HCCL_AMD_ALGO_RHD, AllReduceRhd},
    {HCCL_AMD_OP_ALLREDUCE, HCCL_AMD_ALGO_NHR, AllReduceNhr},
    {HCCL_AMD_OP_ALLREDUCE, HCCL_AMD_ALGO_ORDER_PRESERVED, AllReduceTree},
    {HCCL_AMD_OP_ALLREDUCE, HCCL_AMD_ALGO_MESH_CHUNK, AllReduceMeshChunk},
    {HCCL_AMD_OP_REDUCE_SCATTER, HCCL_AMD_ALGO_MESH_ONESHOT, ReduceScatterMesh},
    {HCCL_AMD_OP_REDUCE_SCATTER, HCCL_AMD_ALGO_NHR, ReduceScatterNhr},
    {HCCL_AMD_OP_REDUCE_SCATTER, HCCL_AMD_ALGO_RING, ReduceScatterRing},
    {HCCL_AMD_OP_REDUCE_SCATTER, HCCL_AMD_ALGO_ORDER_PRESERVED, ReduceScatterTree},
    {HCCL_AMD_OP_REDUCE_SCATTER, HCCL_AMD_ALGO_MESH_CHUNK, ReduceScatterMeshChunk},
    // the only AICPU template of ReduceScatterV (reduce_scatter_v_auto_selector.cc:180-197)
    {HCCL_AMD_OP_REDUCE_SCATTER_V, HCCL_AMD_ALGO_MESH_ONESHOT, ReduceScatterVMesh},
    {HCCL_AMD_OP_REDUCE, HCCL_AMD_ALGO_MESH_ONESHOT, ReduceOneShot},
    {HCCL_AMD_OP_REDUCE, HCCL_AMD_ALGO_MESH_TWOSHOT, ReduceTwoShot},
    {HCCL_AMD_OP_REDUCE, HCCL_AMD_ALGO_NHR, ReduceNhr},
    {HCCL_AMD_OP_ALLGATHER, HCCL_AMD_ALGO_MESH_ONESHOT, AllGatherMesh},
    {HCCL_AMD_OP_ALLGATHER, HCCL_AMD_ALGO_RING, AllGatherRing},
    {HCCL_AMD_OP_BROADCAST, HCCL_AMD_ALGO_MESH_TWOSHOT, BroadcastTwoShot},
    {HCCL_AMD_OP_ALLTOALL, HCCL_AMD_ALGO_MESH_ONESHOT, AllToAllMesh},
    {HCCL_AMD_OP_SCATTER, HCCL_AMD_ALGO_MESH_ONESHOT, ScatterMesh},
    {HCCL_AMD_OP_ALLGATHER_V, HCCL_AMD_ALGO_MESH_ONESHOT, AllGatherVMesh},
    {HCCL_AMD_OP_BARRIER, HCCL_AMD_ALGO_NHR, BarrierNhr},
    {HCCL_AMD_OP_BARRIER, HCCL_AMD_ALGO_MESH_ONESHOT, BarrierMesh},
};

// The algorithm a call runs: the requested one after every substitution. What is left without a generator is refused.
int32_t ResolveAlgo(const ScheduleParams& p)
{
    if (p.opType == HCCL_AMD_OP_REDUCE_SCATTER_V) return HCCL_AMD_ALGO_MESH_ONESHOT;
    if (p.opType == HCCL_AMD_OP_BROADCAST) return HCCL_AMD_ALGO_MESH_TWOSHOT;  // data movement only: one schedule
    if (p.opType == HCCL_AMD_OP_ALLTOALL) return HCCL_AMD_ALGO_MESH_ONESHOT;   // likewise
    if (p.opType == HCCL_AMD_OP_SCATTER || p.opType == HCCL_AMD_OP_ALLGATHER_V) return HCCL_AMD_ALGO_MESH_ONESHOT;
    if (p.opType == HCCL_AMD_OP_BARRIER) {
        // the reference's AICPU selection is AicpuBarrierSoleNHR; its Mesh1D template for the two mesh families
        const bool mesh = p.algo == HCCL_AMD_ALGO_MESH_ONESHOT || p.algo == HCCL_AMD_ALGO_MESH_TWOSHOT;
        return mesh ? HCCL_AMD_ALGO_MESH_ONESHOT : HCCL_AMD_ALGO_NHR;
    }
    int32_t algo = p.algo;
    const uint64_t bytes = p.count * p.elemSize;
    if (algo == HCCL_AMD_ALGO_AUTO) algo = SelectAlgo(p.opType, p.nRanks, bytes, p.special);
    // The one-sided IPC collectives run as one kernel per executor loop, not as IR; their IR twins (same orders, same
    // bits) are the two-shot AllReduce / Reduce and the mesh ReduceScatter, which also run when the IPC path cannot.
    if (algo == HCCL_AMD_ALGO_IPC_TWOSHOT) algo = HCCL_AMD_ALGO_MESH_TWOSHOT;
    if (algo == HCCL_AMD_ALGO_IPC) algo = SelectAlgo(p.opType, p.nRanks, bytes, p.special);
    if (p.nRanks == 1) return algo;  // one rank copies, whatever the family
    const bool ring = algo == HCCL_AMD_ALGO_RING, rhd = algo == HCCL_AMD_ALGO_RHD;
    switch (p.opType) {
        case HCCL_AMD_OP_ALLREDUCE: return rhd && !IsPow2(p.nRanks) ? HCCL_AMD_ALGO_RING : algo;
        case HCCL_AMD_OP_REDUCE_SCATTER:
            return algo == HCCL_AMD_ALGO_MESH_TWOSHOT || rhd ? HCCL_AMD_ALGO_MESH_ONESHOT : algo;
        case HCCL_AMD_OP_REDUCE:
            return ring || rhd || algo == HCCL_AMD_ALGO_ORDER_PRESERVED || algo == HCCL_AMD_ALGO_MESH_CHUNK
                       ? HCCL_AMD_ALGO_MESH_TWOSHOT
                       : algo;
        case HCCL_AMD_OP_ALLGATHER: return ring ? algo : HCCL_AMD_ALGO_MESH_ONESHOT;
        default: return algo;
    }
}

}  // namespace

int32_t SelectAlgo(int32_t opType, uint32_t nRanks, uint64_t bytes, bool special)
{
    // DEFAULT_RANK_SIZE = 8.0 (auto_selector_base.h:28): AllReduce ratio 8/n/n, ReduceScatter (8/n)^2, in double
    const double n = nRanks == 0 ? 8.0 : double(nRanks);
    switch (opType) {
        case HCCL_AMD_OP_ALLREDUCE:
            if (bytes <= kOneShotMaxBytes) return HCCL_AMD_ALGO_MESH_ONESHOT;
            if (!special && double(bytes) * (8.0 / n / n) > double(32ull << 20)) return HCCL_AMD_ALGO_MESH_CHUNK;
            return HCCL_AMD_ALGO_MESH_TWOSHOT;
        case HCCL_AMD_OP_REDUCE_SCATTER:
            if (!special && double(bytes) * (8.0 / n) * (8.0 / n) > double(16ull << 20)) {
                return HCCL_AMD_ALGO_MESH_CHUNK;
            }
            return HCCL_AMD_ALGO_MESH_ONESHOT;
        case HCCL_AMD_OP_REDUCE:
            return bytes < kOneShotMaxBytes ? HCCL_AMD_ALGO_MESH_ONESHOT : HCCL_AMD_ALGO_MESH_TWOSHOT;
        case HCCL_AMD_OP_ALLGATHER: return HCCL_AMD_ALGO_MESH_ONESHOT;
        case HCCL_AMD_OP_BROADCAST: return HCCL_AMD_ALGO_MESH_TWOSHOT;  // broadcast_auto_selector.cc:233-246
        case HCCL_AMD_OP_ALLTOALL: return HCCL_AMD_ALGO_MESH_ONESHOT;   // ins_temp_all_to_all_v_mesh_1D.cc
        case HCCL_AMD_OP_SCATTER: return HCCL_AMD_ALGO_MESH_ONESHOT;    // ins_temp_scatter_mesh_1D.cc
        case HCCL_AMD_OP_ALLGATHER_V: return HCCL_AMD_ALGO_MESH_ONESHOT;  // ins_temp_all_gather_v_mesh_1D.cc
        case HCCL_AMD_OP_BARRIER: return HCCL_AMD_ALGO_NHR;  // AicpuBarrierSoleNHR (barrier_auto_selector.cc)
        default: return HCCL_AMD_ALGO_AUTO;
    }
}

int BuildSchedule(const ScheduleParams& p, Schedule* out)
{
    if (p.nRanks == 0 || p.rank >= p.nRanks || p.elemSize == 0 || p.nRanks > HCCL_AMD_IR_MAX_SRC) {
        return HCCL_E_PARA;
    }
    const bool rooted = p.opType == HCCL_AMD_OP_REDUCE || p.opType == HCCL_AMD_OP_BROADCAST ||
                        p.opType == HCCL_AMD_OP_SCATTER;
    if (rooted && p.root >= p.nRanks) return HCCL_E_PARA;
    const bool agv = p.opType == HCCL_AMD_OP_ALLGATHER_V;
    const bool v = p.opType == HCCL_AMD_OP_REDUCE_SCATTER_V || agv;
    if (v && (p.counts.size() != p.nRanks || p.displs.size() != p.nRanks)) return HCCL_E_PARA;
    const bool a2a = p.opType == HCCL_AMD_OP_ALLTOALL;
    if (a2a && (p.counts.size() != p.nRanks || p.displs.size() != p.nRanks || p.recvCounts.size() != p.nRanks ||
                p.recvDispls.size() != p.nRanks)) {
        return HCCL_E_PARA;
    }
    const int32_t algo = ResolveAlgo(p);
    Builder b;
    if (p.nRanks == 1) {
        // SingleRankProc (op_common.cc:3042-3098): a copy when the buffers differ (a Broadcast has one buffer).
        if (a2a) {
            b.Copy(Out(p.recvDispls[0]), In(p.displs[0]), p.counts[0]);
        } else if (agv) {
            if (!p.inPlace) b.Copy(Out(p.displs[0]), In(0), p.counts[0]);
        } else if (p.opType != HCCL_AMD_OP_BROADCAST && p.opType != HCCL_AMD_OP_BARRIER) {
            b.Copy(Out(0), In(v ? p.displs[0] : 0), v ? p.counts[0] : p.count);
        }
    } else {
        Generator gen = nullptr;
        for (const GeneratorEntry& e : kGenerators) {
            if (e.opType == p.opType && e.algo == algo) gen = e.gen;
        }
        if (gen == nullptr) return HCCL_E_PARA;
        gen(p, b);
    }
    out->ops = std::move(b.ops);
    out->algo = algo;
    out->scratchElems = b.scratchHigh;
    return HCCL_SUCCESS;
}

}  // namespace hccl_amd
