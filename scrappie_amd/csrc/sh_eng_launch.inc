/* sh_eng_launch.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * launch-group construction (tiles, metadata, schedules) and the kernel dispatch helpers: which instantiation of a kernel family runs for a layer's
 * sizes and switches, each launched through launch_k (scrappie_hip.hip). */

/* ------------------------------------------------------------------ */
/* launch-group construction                                            */
/* ------------------------------------------------------------------ */
struct MetaPtrs { ShMeta md; const long long *seq_off, *hp_off, *bases_off; ShGruLanes lanes, lanes1; ShGruPairs pairs, pairs2; const ShGruSegD *vseg, *vlseg; const int *vloff; ShDwellArgs dw; };

/* Bytes of bases reserved for a read whose path has nentry entries.  Plain stitching: k of the first k-mer + at most k per later entry (k <= 5), a
 * bound.  With the dwell correction a call has no bound of that kind: a homopolymer of hdwell samples gets round(hdwell / scale) bases, and the scale
 * -- about the mean dwell of a step -- may come out small against one long dwell.  Over a read the homopolymers get at most sum(dwell) / scale +
 * nentry / 2 bases (half a base of rounding each, a run owns two entries), so SH_DWELL_PER_ENTRY = 10 bytes an entry hold every read whose scale is at
 * least 2 / 9 of its mean dwell: 5 as before, 4.5 for the dwells, 0.5 for the rounding.  A read outside that is the device's to notice (sh_dwell.h
 * counts against the reservation before it stores) and the host's to stitch. */
#define SH_DWELL_PER_ENTRY 10
static long long bases_reservation(long long per_entry, long long nentry) { return (per_entry * nentry + 16 + 15) & ~15ll; }
extern "C" size_t scrappie_hip_dwell_capacity(size_t nentry) { return (size_t)bases_reservation(SH_DWELL_PER_ENTRY, (long long)nentry); }

static int build_group(scrappie_hip_engine *e, Slot &sl, Model *m, const uint64_t *offsets, const uint32_t *lengths,
                       size_t n, bool hp_on, MetaPtrs &mp, const DwellJob *dw = nullptr, const PostJob *pj = nullptr) {
    LaunchGroup &lg = sl.lg;
    lg.valid = false;
    lg.n = n; lg.hp_on = hp_on;
    lg.dw = DwellJob();
    if (dw && dw->on) {
        if (m->arch != 3 || dw->off.size() != n || dw->num.size() != n || dw->host.size() != n) return set_err("build_group: %zu reads, dwells of %zu", n, dw->off.size());
        lg.dw = *dw;
    }
    lg.post = PostJob(); lg.npost = 0;
    if (pj && pj->on) {
        if (m->arch != 1 || pj->dst.size() != n) return set_err("build_group: base probabilities of %zu reads for a group of %zu (flip-flop models only)", pj->dst.size(), n);
        lg.post = *pj;
    }
    lg.ntile = (n + 15) / 16; lg.npad = lg.ntile * 16;
    const int st = m->stride;
    std::vector<int> T(n);
    for (size_t i = 0; i < n; i++)
        T[i] = (lengths[i] >= m->min_samples) ? (int)((lengths[i] + st - 1) / st) : 0;
    lg.order.assign(lg.npad, -1);
    std::vector<int> idx(n);
    std::iota(idx.begin(), idx.end(), 0);
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return T[a] > T[b]; });
    for (size_t i = 0; i < n; i++) lg.order[i] = idx[i];
    lg.rT.assign(lg.npad, 0); lg.rN.assign(lg.npad, 0);
    lg.seq_off.assign(lg.npad, 0); lg.hp_off.assign(lg.npad, 0); lg.bases_off.assign(lg.npad, 0);
    long long nbases = 0;
    /* bases a read can give: k of the first k-mer + at most k per later path entry (k <= 5; CRF: one per block), + 1 */
    const long long per_entry = (m->arch == 1) ? 1 : (lg.dw.on ? (e->dbg_dwell_tight ? 0 : SH_DWELL_PER_ENTRY) : 5);      /* (test hook: 16 bytes a read, so that calls do outgrow them) */
    std::vector<unsigned long long> sig_off(lg.npad, 0);
    std::vector<int> tile_T(lg.ntile, 0);
    std::vector<long long> &tile_boff = lg.tile_boff;
    tile_boff.assign(lg.ntile, 0);
    long long ncb = 0, nseq = 0, nhp = 0;
    for (size_t i = 0; i < lg.npad; i++) {
        const int o = lg.order[i];
        if (o >= 0 && T[o] > 0) {
            lg.rT[i] = T[o]; lg.rN[i] = (int)lengths[o]; sig_off[i] = offsets[o];
        }
        lg.hp_off[i] = nhp; nhp += lg.rT[i];
        lg.bases_off[i] = nbases; nbases += lg.rT[i] ? bases_reservation(per_entry, (long long)lg.rT[i] + 1) : 0;
        tile_T[i >> 4] = std::max(tile_T[i >> 4], lg.rT[i]);
    }
    for (size_t t = 0; t < lg.ntile; t++) { tile_boff[t] = ncb; ncb += tile_T[t]; }
    /* decoded paths: tile-interleaved, entry t of read b of a tile at tile base + t * SH_SEQ_STRIDE + b (sh_kernels.h) */
    for (size_t t = 0; t < lg.ntile; t++) {
        for (int b = 0; b < 16; b++) lg.seq_off[t * 16 + b] = nseq + b;
        nseq += tile_T[t] ? ((long long)tile_T[t] + 1) * SH_SEQ_STRIDE : 0;
    }
    lg.ncb = ncb; lg.nseq = nseq; lg.nhp = nhp; lg.nbases_cap = nbases;
    ShGruSchedule sched;
    sh_lane_schedule(tile_T.data(), lg.ntile, e->ncu, 2, sched, e->handover);   /* GRU and LSTM kernels: two lanes per workgroup */
    lg.gru_nwg = sched.nwg;
    ShGruSchedule sched1;
    sh_lane_schedule(tile_T.data(), lg.ntile, e->ncu, 1, sched1, e->handover);  /* projection + recurrence kernel: one lane per workgroup */
    lg.gru1_nwg = sched1.nwg;
    { long long nlive = 0; int tmax = 0; for (int t : tile_T) { nlive += t > 0; tmax = std::max(tmax, t); }
      /* One or two tiles per workgroup: a launch lasts its longest lane's steps, and a workgroup with one tile steps
       * SH_GRU_TWO_RATIO times faster than one with two (1.9 against 3.2 us per step with every CU busy, 1.35 against
       * 2.65 with a quarter of them idle).  Equal reads: half the steps per lane beat that.  Mixed lengths whose longest
       * tile sets both capacities do not (6000 reads of U{1000..40000} samples: 54 against 109 ms for five layers).
       * (k_gru_proj<.., 2> keeps two block counts in one register: tmax < 65536.) */
      const int w1 = sched1.wg_iter.empty() ? 0 : *std::max_element(sched1.wg_iter.begin(), sched1.wg_iter.end());
      const int w2 = sched.wg_iter.empty() ? 0 : *std::max_element(sched.wg_iter.begin(), sched.wg_iter.end());
      lg.gru_two = nlive > e->ncu && tmax < 65536 && (double)w2 * tun().gru_two_ratio < (double)w1;
      if (e->dbg_gru_tiles == 1) lg.gru_two = false;
      if (e->dbg_gru_tiles == 2 && tmax < 65536) lg.gru_two = true; }
    /* k_gru_proj32: tiles stepped two at a time (neighbours in the length order; a tile of 2^18 blocks or more alone: the
     * kernel addresses both tiles of a pair from one base with 32-bit byte offsets), the pairs laid over the lanes like tiles */
    std::vector<int> pair_tile, pair_T;
    for (size_t t = 0; t < lg.ntile; ) {
        const bool two = t + 1 < lg.ntile && tile_T[t] < (1 << 18) && tile_T[t + 1] > 0;
        pair_tile.push_back((int)t); pair_tile.push_back(two ? (int)t + 1 : -1);
        pair_T.push_back(std::max(tile_T[t], two ? tile_T[t + 1] : 0));
        t += two ? 2 : 1;
    }
    ShGruSchedule sched32;
    sh_lane_schedule(pair_T.data(), pair_T.size(), e->ncu, 1, sched32, e->handover);
    lg.gru32_nwg = sched32.nwg;
    ShGruSchedule sched32b;
    sh_lane_schedule(pair_T.data(), pair_T.size(), e->ncu, 2, sched32b, e->handover);
    lg.gru32x2_nwg = sched32b.nwg;
    std::vector<ShGruSeg> vseg;                  /* decoder, k_viterbi and k_ff_viterbi: one piece of a tile per workgroup */
    sh_piece_schedule(tile_T.data(), lg.ntile, e->dbg_decoder_cus > 0 ? e->dbg_decoder_cus : e->ncu, vseg, e->handover);
    lg.vit_nwg = (int)vseg.size();
    /* k_ff_viterbi_teams: tiles end to end over one lane per workgroup, cut only where a lane is full (the "decoder_cus" debug option
     * alone: the equal pieces the other two kernels get, a lane each) */
    ShGruSchedule vlanes;
    if (e->dbg_decoder_cus > 0 && e->dbg_decoder_lanes <= 0) sh_pieces_as_lanes(vseg, vlanes);
    else sh_decoder_lanes(tile_T.data(), lg.ntile, e->dbg_decoder_lanes > 0 ? e->dbg_decoder_lanes : e->ncu, vlanes, e->handover);
    lg.vit_lane_nwg = vlanes.nwg; lg.vit_lane_nseg = (int)vlanes.seg.size();
    /* pack metadata: [sig_off u64 npad][seq_off i64 npad][hp_off i64 npad][tile_boff i64 ntile][rN i32 npad][rT i32 npad][tile_T i32 ntile] */
    const size_t b_u64 = lg.npad * 8, b_i32 = lg.npad * 4;
    const size_t b_loff = sched.lane_off.size() * 4, b_seg = sched.seg.size() * sizeof(ShGruSeg), b_wit = sched.wg_iter.size() * 4;
    const size_t b_vseg = vseg.size() * sizeof(ShGruSeg);
    const size_t b_vloff = vlanes.lane_off.size() * 4, b_vlseg = vlanes.seg.size() * sizeof(ShGruSeg);
    const size_t b_loff1 = sched1.lane_off.size() * 4, b_seg1 = sched1.seg.size() * sizeof(ShGruSeg);
    const size_t b_loff32 = sched32.lane_off.size() * 4, b_seg32 = sched32.seg.size() * sizeof(ShGruSeg), b_pt = pair_tile.size() * 4;
    const size_t b_loff32b = sched32b.lane_off.size() * 4, b_seg32b = sched32b.seg.size() * sizeof(ShGruSeg);
    const size_t total = 4 * b_u64 + lg.ntile * 8 + 2 * b_i32 + lg.ntile * 4 + 16 + b_seg + b_loff + b_wit + 16 + b_vseg + 16 + b_vlseg + b_vloff + 16 + b_seg1 + b_loff1 +
                         16 + b_seg32 + b_loff32 + b_pt + 16 + b_seg32b + b_loff32b;
    if (sl.h_meta.ensure(total + 16) || sl.d_meta.ensure(total + 16)) return -1;
    char *h = sl.h_meta.as<char>();
    size_t o = 0;
    memcpy(h + o, sig_off.data(), b_u64); const size_t o_sig = o; o += b_u64;
    memcpy(h + o, lg.seq_off.data(), b_u64); const size_t o_seq = o; o += b_u64;
    memcpy(h + o, lg.hp_off.data(), b_u64); const size_t o_hp = o; o += b_u64;
    memcpy(h + o, lg.bases_off.data(), b_u64); const size_t o_bs = o; o += b_u64;
    memcpy(h + o, tile_boff.data(), lg.ntile * 8); const size_t o_tb = o; o += lg.ntile * 8;
    memcpy(h + o, lg.rN.data(), b_i32); const size_t o_n = o; o += b_i32;
    memcpy(h + o, lg.rT.data(), b_i32); const size_t o_t = o; o += b_i32;
    memcpy(h + o, tile_T.data(), lg.ntile * 4); const size_t o_tt = o; o += lg.ntile * 4;
    o = (o + 15) & ~(size_t)15;
    memcpy(h + o, sched.seg.data(), b_seg); const size_t o_seg = o; o += b_seg;
    memcpy(h + o, sched.lane_off.data(), b_loff); const size_t o_loff = o; o += b_loff;
    memcpy(h + o, sched.wg_iter.data(), b_wit); const size_t o_wit = o; o += b_wit;
    o = (o + 15) & ~(size_t)15;
    memcpy(h + o, vseg.data(), b_vseg); const size_t o_vseg = o; o += b_vseg;
    o = (o + 15) & ~(size_t)15;
    memcpy(h + o, vlanes.seg.data(), b_vlseg); const size_t o_vlseg = o; o += b_vlseg;
    memcpy(h + o, vlanes.lane_off.data(), b_vloff); const size_t o_vloff = o; o += b_vloff;
    o = (o + 15) & ~(size_t)15;
    memcpy(h + o, sched1.seg.data(), b_seg1); const size_t o_seg1 = o; o += b_seg1;
    memcpy(h + o, sched1.lane_off.data(), b_loff1); const size_t o_loff1 = o; o += b_loff1;
    o = (o + 15) & ~(size_t)15;
    memcpy(h + o, sched32.seg.data(), b_seg32); const size_t o_seg32 = o; o += b_seg32;
    memcpy(h + o, sched32.lane_off.data(), b_loff32); const size_t o_loff32 = o; o += b_loff32;
    memcpy(h + o, pair_tile.data(), b_pt); const size_t o_pt = o; o += b_pt;
    o = (o + 15) & ~(size_t)15;
    memcpy(h + o, sched32b.seg.data(), b_seg32b); const size_t o_seg32b = o; o += b_seg32b;
    memcpy(h + o, sched32b.lane_off.data(), b_loff32b); const size_t o_loff32b = o; o += b_loff32b;
    hipStream_t ps = e->ev_ok ? e->pstream : e->stream;      /* prologue stream: see run_pipeline */
    if (e->ev_ok) {
        const long long n16 = (long long)((total + 15) / 16);
        hipLaunchKernelGGL(k_upload_words, dim3((unsigned)std::min<long long>((n16 + 255) / 256, 64)), dim3(256), 0, ps, (const u32x4 *)h, sl.d_meta.as<u32x4>(), n16);
    } else HIPCHK(hipMemcpyAsync(sl.d_meta.p, h, total, hipMemcpyHostToDevice, ps));
    char *d = sl.d_meta.as<char>();
    mp.md.sig_off = (const unsigned long long *)(d + o_sig);
    mp.seq_off = (const long long *)(d + o_seq);
    mp.hp_off = (const long long *)(d + o_hp);
    mp.bases_off = (const long long *)(d + o_bs);
    mp.md.tile_boff = (const long long *)(d + o_tb);
    mp.md.rN = (const int *)(d + o_n);
    mp.md.rT = (const int *)(d + o_t);
    mp.md.tile_T = (const int *)(d + o_tt);
    static_assert(sizeof(ShGruSeg) == sizeof(ShGruSegD), "segment layout");
    mp.lanes.seg = (const ShGruSegD *)(d + o_seg);
    mp.lanes.lane_off = (const int *)(d + o_loff);
    mp.lanes.wg_iter = (const int *)(d + o_wit);
    mp.lanes.ntile = (int)lg.ntile;
    mp.vseg = (const ShGruSegD *)(d + o_vseg);
    mp.vlseg = (const ShGruSegD *)(d + o_vlseg);
    mp.vloff = (const int *)(d + o_vloff);
    if (e->d_hstate.ensure(std::max<size_t>(lg.ntile, 1) * 12 * 256 * 4) || sl.d_gflag.ensure((lg.ntile + 1) * 4)) return -1;
    mp.lanes.hstate = e->d_hstate.as<float>();
    mp.lanes.flag = sl.d_gflag.as<unsigned>();
    HIPCHK(hipMemsetAsync(sl.d_gflag.p, 0, (lg.ntile + 1) * 4, ps));
    if (sl.d_bad.ensure(lg.npad * 4)) return -1;
    HIPCHK(hipMemsetAsync(sl.d_bad.p, 0, lg.npad * 4, ps));
    mp.lanes1 = mp.lanes;
    mp.lanes1.seg = (const ShGruSegD *)(d + o_seg1);
    mp.lanes1.lane_off = (const int *)(d + o_loff1);
    mp.lanes1.wg_iter = nullptr;
    mp.pairs.seg = (const ShGruSegD *)(d + o_seg32);
    mp.pairs.lane_off = (const int *)(d + o_loff32);
    mp.pairs.pair_tile = (const int *)(d + o_pt);
    mp.pairs.hstate = mp.lanes.hstate;           /* 3072 floats per pair <= 2 x 6 x 256 per tile */
    mp.pairs.flag = mp.lanes.flag;
    mp.pairs.err = mp.lanes.flag + lg.ntile;
    mp.pairs2 = mp.pairs;
    mp.pairs2.seg = (const ShGruSegD *)(d + o_seg32b);
    mp.pairs2.lane_off = (const int *)(d + o_loff32b);
    mp.dw = ShDwellArgs{};
    if (lg.dw.on) {
        /* the dwell kernel's per-read words in tiled order: [dwell_off i64][prior_num f32][cap i32], behind the metadata on the prologue stream */
        const size_t np = lg.npad, bytes = (np * 16 + 15) & ~(size_t)15;
        if (sl.h_dwmeta.ensure(bytes) || sl.d_dwmeta.ensure(bytes)) return -1;
        long long *hoff = sl.h_dwmeta.as<long long>();
        float *hnum = (float *)(hoff + np);
        int *hcap = (int *)(hnum + np);
        for (size_t i = 0; i < np; i++) {
            const int o2 = lg.order[i];
            const bool live = o2 >= 0 && lg.rT[i] > 0;
            hoff[i] = live ? (long long)lg.dw.off[(size_t)o2] : 0;
            hnum[i] = live ? lg.dw.num[(size_t)o2] : 0.0f;
            hcap[i] = live ? (int)std::min<long long>(bases_reservation(per_entry, (long long)lg.rT[i] + 1), INT32_MAX & ~15) : 0;
        }
        if (e->ev_ok) hipLaunchKernelGGL(k_upload_words, dim3((unsigned)std::min<size_t>((bytes / 16 + 255) / 256, 64)), dim3(256), 0, ps, (const u32x4 *)sl.h_dwmeta.p, sl.d_dwmeta.as<u32x4>(), (long long)(bytes / 16));
        else HIPCHK(hipMemcpyAsync(sl.d_dwmeta.p, sl.h_dwmeta.p, bytes, hipMemcpyHostToDevice, ps));
        char *dd = sl.d_dwmeta.as<char>();
        mp.dw.dwell = lg.dw.d_dwell;
        mp.dw.dwell_off = (const long long *)dd;
        mp.dw.prior_num = (const float *)(dd + np * 8);
        mp.dw.cap = (const int *)(dd + np * 12);
        mp.dw.nd = mp.md.rT;
        mp.dw.ntrail = 1;
    }
    return 0;
}

/* ------------------------------------------------------------------ */
/* kernel dispatch helpers                                              */
/* ------------------------------------------------------------------ */
/* Every launch goes through launch_k (scrappie_hip.hip: the dynamic-LDS limit, once per device and instantiation); run-time sizes and flags become
 * template arguments through pick_int / pick_bool, with a launch's argument list written once; the instrumented forms (STAMP = true, k_gru_conv_stamp)
 * are named where their switch is tested and read back through a StampBuf. */
template <int KQ>
static int launch_affine_k(hipStream_t s, const float *in, float *out, const float *wf, const unsigned *wp, const float *bf,
                           long long ncb, int mtiles) {
    const int mt = pick_mt(mtiles);
    long long gx = std::min<long long>((ncb + 3) / 4, 2048);
    if (gx < 1) gx = 1;
    dim3 grid((unsigned)gx, (unsigned)(mtiles / mt));
    int rc = 0;
    if (pick_int<6, 4, 3, 2, 1>(mt, rc, [&](auto m) { return launch_k<k_affine<KQ, m()>>(grid, dim3(256), 0, s, in, out, wf, wp, bf, ncb, mtiles); })) return rc;
    return set_err("unsupported layer of %d m-tiles", mtiles);
}

template <int KQ>
static int launch_affine_lds_k(hipStream_t s, const float *in, float *out, const float *wf, const unsigned *wp, const float *bf,
                               long long ncb, int mtiles) {
    constexpr int NB = SH_AFF_NB, NTH = SH_AFF_NTH;
    const size_t lds = ((size_t)mtiles * KQ * 256 + (size_t)mtiles * 256) * 4 + 16;
    long long gx = std::min<long long>((ncb + (NTH / 64) * NB - 1) / ((NTH / 64) * NB), 256);
    if (gx < 1) gx = 1;
    /* column groups by fixed striding: measured 4 % faster here than the dynamic hand-out k_ff_lds uses */
    return launch_k<k_affine_lds<KQ, NB, NTH>>(dim3((unsigned)gx), dim3(NTH), lds, s, in, out, wf, wp, bf, ncb, mtiles);
}

/* exact-fp32 MFMAs on the fp32 fragments whatever K: the projection of a layer whose weights are outside the split
 * products' operand range (Model::layer_f32) */
template <int KQ>
static int launch_affine_f32_k(hipStream_t s, const float *in, float *out, const float *wf, const float *bf, long long ncb, int mtiles) {
    const int mt = (mtiles % 6 == 0) ? 6 : (mtiles % 2 == 0) ? 2 : 1;
    long long gx = std::min<long long>((ncb + 3) / 4, 2048);
    if (gx < 1) gx = 1;
    dim3 grid((unsigned)gx, (unsigned)(mtiles / mt));
    int rc = 0;
    if (pick_int<6, 2, 1>(mt, rc, [&](auto m) { return launch_k<k_affine<KQ, m(), true>>(grid, dim3(256), 0, s, in, out, wf, (const unsigned *)nullptr, bf, ncb, mtiles); })) return rc;
    return set_err("unsupported layer of %d m-tiles", mtiles);
}

static int launch_affine(hipStream_t s, int K, const float *in, float *out, const float *wf, const unsigned *wp, const float *bf_nat,
                         const float *bf_acc, long long ncb, int mtiles, bool force_f32 = false) {
    int rc = 0;
    /* (odd K / 16: the ordinary kernel is exact-fp32 already) */
    if (force_f32 && pick_int<2, 4, 6, 8>(K / 16, rc, [&](auto kq) { return launch_affine_f32_k<kq()>(s, in, out, wf, bf_nat, ncb, mtiles); })) return rc;
    if (K % 32 == 0 && (!wp || !bf_acc)) return set_err("layer weights were not cut into pieces (input size %d)", K);
    const float *bf = (K % 32 == 0) ? bf_acc : bf_nat;      /* split products start from the bias in accumulator units */
    /* big layers: LDS-resident weights, input read once */
    const size_t lds_need = ((size_t)mtiles * (K / 16) * 256 + (size_t)mtiles * 256) * 4;
    if (mtiles >= 12 && lds_need <= 150 * 1024 && ncb >= 4096 && !tun().affine_reg &&
        pick_int<1, 2, 4, 6>(K / 16, rc, [&](auto kq) { return launch_affine_lds_k<kq()>(s, in, out, wf, wp, bf, ncb, mtiles); })) return rc;
    if (pick_int<1, 2, 4, 6, 8>(K / 16, rc, [&](auto kq) { return launch_affine_k<kq()>(s, in, out, wf, wp, bf, ncb, mtiles); })) return rc;
    return set_err("unsupported layer input size %d (need 16, 32, 64, 96 or 128)", K);
}

template <int KQ>
static int launch_affine2_k(hipStream_t s, const float *inF, const float *inB, float *out, const unsigned *wF, const unsigned *wB,
                            const float *bf, long long ncb, int mtiles) {
    long long gx = std::min<long long>((ncb + 3) / 4, 2048);
    if (gx < 1) gx = 1;
    /* S / 16 = 2, 4 or 6 m-tiles: two wave quartets per workgroup, each with half of them */
    const int mt = mtiles / 2;
    int rc = 0;
    if (mt * 2 == mtiles &&
        pick_int<3, 2, 1>(mt, rc, [&](auto m) { return launch_k<k_affine2_tanh<KQ, m()>>(dim3((unsigned)gx), dim3(512), 0, s, inF, inB, out, wF, wB, bf, ncb, mtiles); })) return rc;
    return set_err("unsupported joining layer of %d m-tiles", mtiles);
}

static int launch_affine2(hipStream_t s, int K, const float *inF, const float *inB, float *out, const unsigned *wF, const unsigned *wB,
                          const float *bf, long long ncb, int mtiles) {
    int rc = 0;
    if (pick_int<2, 4, 6>(K / 16, rc, [&](auto kq) { return launch_affine2_k<kq()>(s, inF, inB, out, wF, wB, bf, ncb, mtiles); })) return rc;
    return set_err("unsupported bi-GRU size %d (need 32, 64 or 96)", K);
}

static int launch_gru(hipStream_t s, int S, const float *xaff, float *out, const float *resid, const float *sW,
                      const float *sW2, const unsigned *sWp, const unsigned *sW2p, const ShMeta &md, int backward, size_t ntile, const ShGruLanes &lanes, int nwg,
                      bool force_f32 = false) {
    const int NU = S / 16;
    int rc = 0;
    /* production path: two lanes per workgroup walking the lane schedule (sh_sched.h) */
    if (!tun().gru_single && !tun().gru_stamp && tun().gru_debug < 0 && NU <= 6 && S % 32 == 0) {
        if (nwg <= 0) return 0;
        /* arrival counters of tiles cut between lanes: cleared before every launch */
        HIPCHK(hipMemsetAsync(lanes.flag, 0, (size_t)lanes.ntile * 4, s));
        dim3 lgrid((unsigned)nwg);
        const bool stamp = tun().gru_lanes_stamp;
        const bool f32_env = tun().gru_f32 || force_f32;
        if (!stamp && !f32_env) {                  /* production: split products */
            const size_t plds = (size_t)2 * 2 * (NU / 2) * 2 * 64 * 4 * 4;
            if (pick_int<2, 4, 6>(NU, rc, [&](auto nu) { return launch_k<k_gru_split<nu()>>(lgrid, dim3(128 * nu()), plds, s, xaff, out, resid, sWp, sW2p, md, backward, lanes); })) return rc;
            return set_err("unsupported GRU size %d (need 32, 64 or 96 here)", S);
        }
        /* SH_GRU_F32 / SH_GRU_LANES_STAMP: the exact-fp32 MFMA kernel (same schedule), kept as the reference the
         * split products were measured against; the stamped form exists for S = 96 only */
        const size_t lds = (size_t)2 * 2 * NU * 256 * 4;
        static StampBuf st;
        if (!pick_int<2, 4, 6>(NU, rc, [&](auto nu) {
#ifdef SH_EXPERIMENTS
            if constexpr (nu() == 6)
                if (stamp) return launch_k<k_gru_lanes<6, true>>(lgrid, dim3(768), lds, s, xaff, out, resid, sW, sW2, md, backward, lanes, st.dev(4096 * 16 * 8));
#endif
            return launch_k<k_gru_lanes<nu(), false>>(lgrid, dim3(128 * nu()), lds, s, xaff, out, resid, sW, sW2, md, backward, lanes, (unsigned long long *)nullptr);
            })) return set_err("unsupported GRU size %d (need 32, 64 or 96 here)", S);
        if (stamp && NU == 6)
            st.dump_on(7, s, (size_t)nwg * 12 * 8, [&](const unsigned long long *h) {
                for (size_t g : {(size_t)nwg / 2}) for (int w = 0; w < 12; w++) {
                    const unsigned long long *d = &h[(g * 12 + w) * 8];
                    fprintf(stderr, "gru lanes stamp wg %zu wave %2d: phase1 %.0f bar %.0f phase2 %.0f bar %.0f cycles/step (%llu steps)\n",
                            g, w, d[0] / (double)d[4], d[1] / (double)d[4], d[2] / (double)d[4], d[3] / (double)d[4], d[4]);
                }
            });
        return rc;
    }
    /* other sizes, and the instrumented single-tile kernel (SH_GRU_SINGLE / SH_GRU_STAMP / SH_GRU_DEBUG) */
    if (tun().gru_debug >= 0) backward |= tun().gru_debug << 8;
    static StampBuf st1;
    unsigned long long *dbgbuf = tun().gru_stamp ? st1.dev(4096 * 8 * 8) : nullptr;
    if (dbgbuf)         /* before the eighth launch: the stamps of an earlier one */
        st1.dump_on(8, s, ntile * NU * 8, [&](const unsigned long long *h) {
            { unsigned long long first_end = ~0ull, mn = ~0ull, mx = 0; size_t late = 0;
              for (size_t tl = 0; tl < ntile; tl++) { first_end = std::min(first_end, h[tl * NU * 8 + 7]); mn = std::min(mn, h[tl * NU * 8 + 6]); mx = std::max(mx, h[tl * NU * 8 + 7]); }
              for (size_t tl = 0; tl < ntile; tl++) if (h[tl * NU * 8 + 6] >= first_end) late++;
              fprintf(stderr, "residency: %zu tiles, %zu started after the first one finished; span %.1f us\n", ntile, late, (mx - mn) / 100.0); }
            for (size_t tl : {size_t(0)}) for (int w = 0; w < 1; w++) {
                const unsigned long long *d = &h[(tl * NU + w) * 8];
                fprintf(stderr, "stamp tile %zu wave %d: rgemm %.0f zgemm+valu %.0f bar1 %.0f gemm2+valu %.0f bar2 %.0f (cycles/step)\n", tl, w, d[0] / (double)d[5], d[1] / (double)d[5], d[2] / (double)d[5], d[3] / (double)d[5], d[4] / (double)d[5]);
            }
        });
    if (pick_int<2, 4, 6, 8>(NU, rc, [&](auto nu) { return launch_k<k_gru<nu()>>(dim3((unsigned)ntile), dim3(64 * nu()), 0, s, xaff, out, resid, sW, sW2, md, backward, dbgbuf); })) return rc;
    return set_err("unsupported GRU size %d (need 32, 64, 96 or 128)", S);
}

#ifndef SH_FFL_NB
#define SH_FFL_NB 3
#endif
#ifndef SH_FFL_NTH
#define SH_FFL_NTH 512
#endif
/* m-tiles per LDS-resident group of the S1 weight fragments (also fixes the order in which row sums are added) */
static int ff_mtp(int KQ, int mtiles) {
    const size_t per_mt = ((size_t)KQ * 256 + 256) * 4;
    int mt_fit = (int)((156 * 1024) / per_mt);
    mt_fit -= mt_fit % SH_SUM_GROUP;            /* whole row-sum groups per part */
    return std::min(mt_fit, (mtiles + SH_SUM_GROUP - 1) / SH_SUM_GROUP * SH_SUM_GROUP);
}

template <int KQ>
static int launch_ff_lds_k(hipStream_t s, const float *in, float *E, float *sums, const unsigned *wf, const float *bf,
                           long long ncb, int mtiles, int NS, float in_div, float out_div, int ncu) {
    constexpr int NB = SH_FFL_NB, NTH = SH_FFL_NTH;
    const int mtp = ff_mtp(KQ, mtiles);
    const size_t lds = (size_t)mtp * ((size_t)KQ * 256 + 256) * 4 + 16;
    long long gx = std::min<long long>((ncb + (NTH / 64) * NB - 1) / ((NTH / 64) * NB), ncu);
    if (gx < 1) gx = 1;
    const bool dv = out_div != 1.0f;
    const bool stamp = tun().ff_stamp && !dv;      /* cycle stamps of every launch on stderr (tuning aid): the form without the division only */
    static StampBuf st;
    unsigned long long *dbg = stamp ? st.dev(16 * 8) : nullptr;
    if (pick_bool([&](auto d) { return launch_k<k_ff_lds<KQ, NB, NTH, d()>>(dim3((unsigned)gx), dim3(NTH), lds, s, in, E, sums, wf, bf, ncb, mtiles, mtp, NS, in_div, out_div, dbg); }, dv))
        return -1;
    if (stamp)
        st.dump_on(0, s, NTH / 64 * 8, [](const unsigned long long *h) {
            for (int w = 0; w < NTH / 64; w++)
                fprintf(stderr, "ff stamp wave %d: fill %llu  B-load %llu  tiles %llu  sums %llu cycles; %llu m-tiles -> %.0f cycles per m-tile\n", w, h[w * 8], h[w * 8 + 1], h[w * 8 + 2], h[w * 8 + 3], h[w * 8 + 4], (double)h[w * 8 + 2] / (double)h[w * 8 + 4]);
        });
    return 0;
}

static int launch_ff(hipStream_t s, int S, const float *in, float *E, float *sums, const unsigned *wf, const float *bf,
                     long long ncb, int mtiles, int NS, float in_div, float out_div, int ncu) {
    int rc = 0;
    /* large batches: weight fragments in LDS (k_ff_lds); small ones: one wave per column group streaming them from L2 */
    if (ncb >= 8192 && !tun().ff_reg &&
        pick_int<2, 4, 6>(S / 16, rc, [&](auto kq) { return launch_ff_lds_k<kq()>(s, in, E, sums, wf, bf, ncb, mtiles, NS, in_div, out_div, ncu); })) return rc;
    constexpr int NB = SH_FF_NB;
    const int mtp = ff_mtp(S / 16, mtiles);
    const long long gx = (ncb + 4 * NB - 1) / (4 * NB);
    dim3 grid((unsigned)std::max<long long>(gx, 1));
    if (pick_int<2, 4, 6, 8>(S / 16, rc, [&](auto kq) {
            constexpr int KQ = kq();
            return pick_bool([&](auto dv) { return launch_k<k_ff_exp<KQ, NB, dv()>>(grid, dim3(256), 0, s, in, E, sums, wf, bf, ncb, mtiles, mtp, NS, in_div, out_div); },
                             out_div != 1.0f);
        })) return rc;
    return set_err("unsupported size %d", S);
}

/* projection + recurrence in one kernel (k_gru_proj): layer input [ncb][S/16][256] -> layer output, the gate
 * inputs never in HBM.  Needs the layer input as wide as the state (K == S) and S in {32, 64, 96}. */
static bool gru_proj_ok(int K, int S) { return K == S && S % 32 == 0 && S / 16 <= 6; }

/* Where a read's convolution windows end, for the layer that computes its own input (k_gru_conv, ShConvFuse::edge): the
 * index arithmetic of layers.c:209-241 as k_conv_mfma / k_conv_act evaluate it per column, evaluated once per read.
 * out = {mask of the last 32 columns without a regular window (bit j: column T - 1 - j), first column with a right-edge
 * partial window, that window's w, N}.  For a given (t - c0) % nstepC the columns with a regular window are a prefix, so
 * 64 columns are looked at; false if one without lies more than 32 columns from the end (the caller then runs the
 * convolution as its own kernel). */
static bool conv_edge_words(const ShConvGeom &g, int N, int T, int out[4]) {
    out[0] = out[1] = out[2] = out[3] = 0;
    if (T <= 0) return true;
    unsigned irr = 0;
    bool ok = true;
    for (int t = std::max(g.c0, T - 64); t < T; t++) {
        const int kk = (t - g.c0) / g.nstepC, ii = (t - g.c0) - kk * g.nstepC;
        if (!((kk + 1) * g.nstepX <= N - g.shiftX - ii * g.st)) {
            const int j = T - 1 - t;
            if (j >= 32) ok = false; else irr |= 1u << j;
        }
    }
    const int maxCol = (N - g.shiftX) / g.nstepX;
    const int rem = (N - g.shiftX) % g.nstepX;
    const int colR = g.c0 + g.nstepC * (maxCol - 1) + rem / g.st + 1;
    const int startR = g.st - (g.padL + N - g.WL) % g.st - 1;
    out[0] = (int)irr; out[1] = colR + startR / g.st; out[2] = startR; out[3] = N;
    return ok;
}

extern "C" int scrappie_hip_conv_edge_words(int WL, int st, int F, int N, int out[4]) {
    if (WL < 1 || st < 1 || N < 1 || !out) return -1;
    return conv_edge_words(conv_geom(WL, st, F), N, (N + st - 1) / st, out) ? 1 : 0;
}

#ifdef SH_EXPERIMENTS
static int launch_gru_conv(hipStream_t s, int kst, int act, float *out, const unsigned *iW, const float *ib, const unsigned *sW,
                           const unsigned *sW2, const ShMeta &md, int backward, const ShGruLanes &lanes1, int nwg1,
                           const ShGruLanes &lanes2, int nwg2, bool two, const ShConvFuse &cf) {
    const ShGruLanes &lanes = two ? lanes2 : lanes1;
    const int nwg = two ? nwg2 : nwg1;
    if (nwg <= 0) return 0;
    HIPCHK(hipMemsetAsync(lanes.flag, 0, (size_t)lanes.ntile * 4, s));
    const size_t lds = (two ? 2 : 1) * ((size_t)4 * 3 * 2 * 64 * 4 + (size_t)2 * 3 * 6 * 256) * 4;
    dim3 grid((unsigned)nwg);
    if (tun().proj_stamp && two && kst == 3 && !act) {       /* cycle stamps of one launch on stderr (tuning aid) */
        static StampBuf st;
        if (launch_k<k_gru_conv_stamp<2, 3, 0>>(grid, dim3(768), lds, s, out, iW, ib, sW, sW2, md, backward, lanes, cf, st.dev(1024 * 12 * 16))) return -1;
        st.dump_on(3, s, (size_t)nwg * 12 * 16, [&](const unsigned long long *h) {
            for (int w = 0; w < 12; w++) {
                const unsigned long long *d = &h[((size_t)(nwg / 2) * 12 + w) * 16];
                fprintf(stderr, "conv-layer stamp wave %2d (%s): A %.0f bar %.0f B %.0f bar %.0f cycles per double step (%llu steps); chunk+fetch part of B (projection) / reads+MFMA issue (recurrence) %.0f\n", w,
                        w < 6 ? "recurrence" : "projection", d[0] / (double)d[4], d[1] / (double)d[4], d[2] / (double)d[4], d[3] / (double)d[4], d[4], d[5] / (double)d[4]);
            }
        });
        return 0;
    }
    return pick_bool([&](auto t2, auto k3, auto ac) {
        return launch_k<k_gru_conv<t2() ? 2 : 1, k3() ? 3 : 5, ac() ? 1 : 0>>(grid, dim3(768), lds, s, out, iW, ib, sW, sW2, md, backward, lanes, cf);
    }, two, kst == 3, act != 0);
}
#endif
static int launch_gru_proj(hipStream_t s, int S, const float *in, float *out, const float *resid, const unsigned *iW, const float *ib,
                           const unsigned *sW, const unsigned *sW2, const ShMeta &md, int backward, const ShGruLanes &lanes1, int nwg1,
                           const ShGruLanes &lanes2, int nwg2, bool two) {
    /* two tiles per workgroup (every wave steps both inside each barrier interval) as soon as there are more tiles
     * than workgroups; else one tile per workgroup, one workgroup per CU */
    const ShGruLanes &lanes = two ? lanes2 : lanes1;
    const int nwg = two ? nwg2 : nwg1;
    if (nwg <= 0) return 0;
    HIPCHK(hipMemsetAsync(lanes.flag, 0, (size_t)lanes.ntile * 4, s));
    const int NU = S / 16;
    size_t lds = (two ? 2 : 1) * ((size_t)4 * (NU / 2) * 2 * 64 * 4 + (size_t)2 * 3 * NU * 256) * 4;
    /* residual layers: + the ring of three input columns per tile slot, wherever it fits (gru_proj_body's RLDS, the same test) */
    if (resid && SH_RESID_LDS && lds + (size_t)(two ? 2 : 1) * 3 * NU * 256 * 4 <= 160 * 1024) lds += (size_t)(two ? 2 : 1) * 3 * NU * 256 * 4;
    dim3 grid((unsigned)nwg);
    unsigned long long *const no_dbg = nullptr;
    int rc = 0;
#ifdef SH_EXPERIMENTS
    /* S = 96, two tiles per workgroup: the form with the matrix work and the elementwise work on different waves (k_gru_mx, sh_gru_mx.h);
     * measured 6 % slower than k_gru_proj (profiles/r5_gru_mx.txt), so it runs only on SH_GRU_MX=1, and only in the experiments build */
    static const bool mx_on = [] { const char *v = getenv("SH_GRU_MX"); return v && atoi(v) != 0; }();
    if (mx_on && NU == 6 && two) {
        static const bool mx_stamp = getenv("SH_MX_STAMP") != nullptr;      /* cycle stamps of the seventh launch on stderr (tuning aid) */
        if (mx_stamp && !resid) {
            static StampBuf st;
            if (launch_k<k_gru_mx<false, true>>(grid, dim3(1024), lds, s, in, out, resid, iW, ib, sW, sW2, md, backward, lanes, st.dev((size_t)1024 * 16 * 10))) return -1;
            st.dump_on(7, s, (size_t)nwg * 16 * 10, [&](const unsigned long long *hb) {
                for (int w = 0; w < 16; w++) {
                    const unsigned long long *d = &hb[((size_t)(nwg / 2) * 16 + w) * 10];
                    const double n = (double)std::max<unsigned long long>(d[8], 1);
                    fprintf(stderr, "mx stamp wave %2d (%s): P1 %.0f +bar %.0f | P2 %.0f +bar %.0f | P3 %.0f +bar %.0f | P4 %.0f +bar %.0f cycles per double step (%llu steps)\n", w,
                            w < 6 ? "recurrence " : w < 12 ? "projection " : "elementwise", d[0] / n, d[1] / n, d[2] / n, d[3] / n, d[4] / n, d[5] / n, d[6] / n, d[7] / n, d[8]);
                }
            });
            return 0;
        }
        if (pick_bool([&](auto rs) { return launch_k<k_gru_mx<rs()>>(grid, dim3(1024), lds, s, in, out, resid, iW, ib, sW, sW2, md, backward, lanes, no_dbg); }, resid != nullptr))
            return -1;
        HIPCHK(hipGetLastError());
        return 0;
    }
    const bool stamp = tun().proj_stamp && NU == 6 && two && !resid;     /* cycle stamps of one launch on stderr (tuning aid) */
    const bool free_run = SH_GRU_FREE_DEFAULT ? !tun().gru_barrier : tun().gru_free;
    if (free_run) {
        /* no s_barrier in the step loop: projection team free running on a ring of three blocks (k_gru_free) */
        const size_t flds = (two ? 2 : 1) * ((size_t)4 * (NU / 2) * 2 * 64 * 4 + (size_t)3 * 3 * NU * 256) * 4 + 64;
        if (stamp) {
            static StampBuf st;
            if (launch_k<k_gru_free<6, 2, false, true>>(grid, dim3(768), flds, s, in, out, resid, iW, ib, sW, sW2, md, backward, lanes, st.dev(1024 * 12 * 16))) return -1;
            st.dump_on(7, s, (size_t)nwg * 12 * 16, [&](const unsigned long long *h) {
                for (int w = 0; w < 12; w++) {
                    const unsigned long long *d = &h[((size_t)(nwg / 2) * 12 + w) * 16];
                    if (w < 6) fprintf(stderr, "free stamp wave %2d (recurrence): work %.0f, waiting for gate inputs %.0f, for r*h of all waves %.0f, for h of all waves %.0f cycles per double step (%llu steps)\n",
                                       w, d[0] / (double)d[4], d[1] / (double)d[4], d[2] / (double)d[4], d[3] / (double)d[4], d[4]);
                    else fprintf(stderr, "free stamp wave %2d (projection): work %.0f, waiting for the column's pieces %.0f, for a free ring slot %.0f cycles per double step (%llu steps)\n",
                                 w, d[0] / (double)d[4], d[1] / (double)d[4], d[2] / (double)d[4], d[4]);
                }
            });
            return 0;
        }
        if (pick_int<2, 4, 6>(NU, rc, [&](auto nu) {
                constexpr int N = nu();
                return pick_bool([&](auto t2, auto rs) {
                    return launch_k<k_gru_free<N, t2() ? 2 : 1, rs(), false>>(grid, dim3(128 * N), flds, s, in, out, resid, iW, ib, sW, sW2, md, backward, lanes, no_dbg);
                }, two, resid != nullptr);
            })) return rc;
        return set_err("unsupported GRU size %d (need 32, 64 or 96 here)", S);
    }
    if (stamp) {
        static StampBuf st;
        if (launch_k<k_gru_proj<6, 2, false, true>>(grid, dim3(768), lds, s, in, out, resid, iW, ib, sW, sW2, md, backward, lanes, st.dev(1024 * 12 * 16))) return -1;
        st.dump_on(7, s, (size_t)nwg * 12 * 16, [&](const unsigned long long *h) {
            for (int w = 0; w < 12; w++) {
                const unsigned long long *d = &h[((size_t)(nwg / 2) * 12 + w) * 16];
                fprintf(stderr, "proj stamp wave %2d (%s): A %.0f bar %.0f B %.0f bar %.0f cycles per double step (%llu steps)", w, w < 6 ? "recurrence" : "projection",
                        d[0] / (double)d[4], d[1] / (double)d[4], d[2] / (double)d[4], d[3] / (double)d[4], d[4]);
                if (w < 6) fprintf(stderr, "; inside B: reads+MFMA issue %.0f, logistic z %.0f, tanh+blend %.0f, store+bookkeeping %.0f, cut+publish %.0f",
                                   d[5] / (double)d[4], d[6] / (double)d[4], d[7] / (double)d[4], d[8] / (double)d[4], d[9] / (double)d[4]);
                fprintf(stderr, "\n");
            }
        });
        return 0;
    }
#endif
    /* residual layers have a kernel of their own (k_gru_proj_res: another register budget), without the stamps' argument */
    if (pick_int<2, 4, 6>(NU, rc, [&](auto nu) {
            constexpr int N = nu();
            return pick_bool([&](auto t2) {
                constexpr int NT = t2() ? 2 : 1;
                if (resid) return launch_k<k_gru_proj_res<N, NT>>(grid, dim3(128 * N), lds, s, in, out, resid, iW, ib, sW, sW2, md, backward, lanes);
                return launch_k<k_gru_proj<N, NT, false>>(grid, dim3(128 * N), lds, s, in, out, resid, iW, ib, sW, sW2, md, backward, lanes, no_dbg);
            }, two);
        })) return rc;
    return set_err("unsupported GRU size %d (need 32, 64 or 96 here)", S);
}

#ifdef SH_EXPERIMENTS
#ifndef SH_GRU32_DEFAULT
#define SH_GRU32_DEFAULT 0        /* 1: recurrent layers of S = 96 run k_gru_proj32 unless SH_GRU16 is set; 0: k_gru_proj unless SH_GRU32 is set */
#endif
static int use_gru32(const scrappie_hip_engine *e) {      /* 0: 16-read tiles; 1: k_gru_proj32; 2: k_gru_proj32x2 (SH_GRU32=2) */
    if (e->dbg_gru32 >= 0) return e->dbg_gru32;
    if (SH_GRU32_DEFAULT ? tun().gru16 : !tun().gru32) return 0;
    const char *v = getenv("SH_GRU32");
    return (v && atoi(v) == 2) ? 2 : (SH_GRU32_DEFAULT ? SH_GRU32_DEFAULT : 1);
}
static const char *const g32_role[8] = {"R0 chain", "R1 chain", "R2 chain", "C cand-proj", "G0 z/r", "G1 z/r", "G2 z/r", "L loader"};
/* one recurrent layer of S = 96 on tiles of 32 reads (k_gru_proj32, sh_gru32.h) */
static int launch_gru_proj32x2(hipStream_t s, const float *in, float *out, bool resid, const unsigned *iW, const float *ib, const unsigned *sW,
                               const unsigned *sW2, const ShMeta &md, int backward, const ShGruPairs &pairs, int nwg, size_t ntile) {
    if (nwg <= 0) return 0;
    HIPCHK(hipMemsetAsync(pairs.flag, 0, ntile * 4, s));
    const size_t lds = (size_t)SH_G32X2_LDS_WORDS * 4;
    dim3 grid((unsigned)nwg);
    if (tun().gru32_stamp && !resid) {
        static StampBuf st;
        if (launch_k<k_gru_proj32x2<false, true>>(grid, dim3(512), lds, s, in, out, iW, ib, sW, sW2, md, backward, pairs, st.dev(1024 * 8 * 16))) return -1;
        st.dump_on(7, s, (size_t)nwg * 8 * 16, [&](const unsigned long long *h) {
            for (int w = 0; w < 8; w++) {
                const unsigned long long *d = &h[((size_t)(nwg / 2) * 8 + w) * 16];
                fprintf(stderr, "gru32x2 stamp wave %d (%s): work %.0f bar %.0f cycles per interval (%llu intervals = one tile-step of 32 reads each)\n", w, g32_role[w],
                        d[0] / (double)d[4], d[1] / (double)d[4], d[4]);
            }
        });
        return 0;
    }
    return pick_bool([&](auto rs) { return launch_k<k_gru_proj32x2<rs(), false>>(grid, dim3(512), lds, s, in, out, iW, ib, sW, sW2, md, backward, pairs, (unsigned long long *)nullptr); }, resid);
}
static int launch_gru_proj32(hipStream_t s, const float *in, float *out, bool resid, const unsigned *iW, const float *ib, const unsigned *sW,
                             const unsigned *sW2, const ShMeta &md, int backward, const ShGruPairs &pairs, int nwg, size_t ntile) {
    if (nwg <= 0) return 0;
    HIPCHK(hipMemsetAsync(pairs.flag, 0, ntile * 4, s));
    const size_t lds = (size_t)SH_G32_LDS_WORDS * 4;
    dim3 grid((unsigned)nwg);
    if (tun().gru32_stamp && !resid) {       /* cycle stamps of one launch on stderr (tuning aid) */
        static StampBuf st;
        if (launch_k<k_gru_proj32<false, true>>(grid, dim3(512), lds, s, in, out, iW, ib, sW, sW2, md, backward, pairs, st.dev(1024 * 8 * 16))) return -1;
        st.dump_on(7, s, (size_t)nwg * 8 * 16, [&](const unsigned long long *h) {
            for (int w = 0; w < 8; w++) {
                const unsigned long long *d = &h[((size_t)(nwg / 2) * 8 + w) * 16];
                fprintf(stderr, "gru32 stamp wave %d (%s): A %.0f bar %.0f B %.0f bar %.0f cycles per step (%llu steps)", w, g32_role[w],
                        d[0] / (double)d[4], d[1] / (double)d[4], d[2] / (double)d[4], d[3] / (double)d[4], d[4]);
                if (w < 3) fprintf(stderr, "; A: reads+r products %.0f, logistic*h %.0f, cut+write %.0f; B: reads+candidate products %.0f, z/tanh/blend %.0f, store %.0f, cut+write %.0f",
                                   d[5] / (double)d[4], d[6] / (double)d[4], d[7] / (double)d[4], d[8] / (double)d[4], d[9] / (double)d[4], d[10] / (double)d[4], d[11] / (double)d[4]);
                fprintf(stderr, "\n");
            }
        });
        return 0;
    }
    return pick_bool([&](auto rs) { return launch_k<k_gru_proj32<rs(), false>>(grid, dim3(512), lds, s, in, out, iW, ib, sW, sW2, md, backward, pairs, (unsigned long long *)nullptr); }, resid);
}

#endif
static int launch_lstm(hipStream_t s, int S, const float *xaff, float *out, const unsigned *sW, const float *pf,
                       const ShMeta &md, int backward, const ShGruLanes &lanes, int nwg) {
    if (nwg <= 0) return 0;
    HIPCHK(hipMemsetAsync(lanes.flag, 0, (size_t)lanes.ntile * 4, s));
    int rc = 0;
    if (pick_int<2, 4, 6>(S / 16, rc, [&](auto nu) { return launch_k<k_lstm_lanes<nu()>>(dim3((unsigned)nwg), dim3(128 * nu()), 0, s, xaff, out, sW, pf, md, backward, lanes); })) return rc;
    return set_err("unsupported LSTM size %d (need 32, 64 or 96)", S);
}

/* projection + LSTM recurrence in one kernel (k_lstm_proj): needs the layer input as wide as the state */
static int launch_lstm_proj(hipStream_t s, int S, int I, const float *in, float *out, const unsigned *iW, const float *ib,
                            const unsigned *sW, const float *pf, const ShMeta &md, int backward, const ShGruLanes &lanes, int nwg) {
    if (nwg <= 0) return 0;
    HIPCHK(hipMemsetAsync(lanes.flag, 0, (size_t)lanes.ntile * 4, s));
    const int NU = S / 16;
    const size_t lds = ((size_t)4 * (NU / 2) * 2 * 64 * 4 + (size_t)2 * 4 * NU * 256 + (size_t)3 * NU * 256) * 4;
    if (I != S && I != 16) return set_err("unsupported LSTM input width %d", I);
    int rc = 0;
    if (pick_int<2, 4, 6>(NU, rc, [&](auto nu) {
            constexpr int N = nu();
            return pick_bool([&](auto wide) { return launch_k<k_lstm_proj<N, wide() ? N : 1>>(dim3((unsigned)nwg), dim3(128 * N), lds, s, in, out, iW, ib, sW, pf, md, backward, lanes); },
                             I == S);
        })) return rc;
    return set_err("unsupported LSTM size %d (need 32, 64 or 96)", S);
}

static size_t viterbi_lds_bytes(int NH) {
    const int nskip = NH / 16, nslip = std::max(NH / 64, 1);
    return (size_t)NH * 16 * 4 * 2 + (size_t)nskip * 16 * 8 + (size_t)nslip * 16 * 8 + 2 * 16 * 16 * 8;
}

static int launch_viterbi(hipStream_t s, int NH, const ShVitArgs &a, const ShMeta &md, size_t nwg) {
    const size_t lds = viterbi_lds_bytes(NH);
    if (nwg == 0) return 0;
    /* the log-posterior transform is compiled in (exp values + sums in, log always) or out (final log-posterior in) */
    const bool fin = a.sums != nullptr, slip = a.use_slip != 0, skip0 = a.skip_pen == 0.0f;
    if (fin && !a.want_log) return set_err("decode: exp-value input implies log output");
    /* nth threads per workgroup, each with ppt quads of states */
    const auto go = [&](auto nth, auto ppt) {
        constexpr int NTH = nth(), PPT = ppt();
        return pick_bool([&](auto fi, auto sl, auto sk) { return launch_k<k_viterbi<NTH, PPT, fi(), sl(), sk()>>(dim3((unsigned)nwg), dim3(NTH), lds, s, a, md); },
                         fin, slip, skip0);
    };
    switch (NH) {
    case 64: return go(int_c<256>(), int_c<1>());
    case 256: return go(int_c<256>(), int_c<4>());
    case 1024:
#ifdef SH_EXPERIMENTS
        if (getenv("SH_VIT_1024")) return go(int_c<1024>(), int_c<4>());      /* sixteen waves of four quads each (four waves per SIMD at 128 VGPRs): see DESIGN.md section 5 */
#endif
        return go(int_c<512>(), int_c<8>());
    default: return set_err("unsupported transducer state count %d (need 4^3, 4^4 or 4^5 k-mers)", NH);
    }
}

/* S1 inside the decoder.  Two teams of waves (k_ff_viterbi_teams: an S1 producer team, a decoder team, scores updated in place) wherever
 * the slip move is off; the eight do-everything waves of k_ff_viterbi with it, under SH_FV_SINGLE=1 and under the "fv_single" debug option
 * (the parity tests compare the two forms bit for bit). */
static int launch_ff_viterbi(hipStream_t s, const ShFfArgs &f, const ShVitArgs &a, const ShMeta &md, size_t nwg, bool single) {
    const size_t lds = (size_t)SH_FV_LDS_FLOATS * 4;
    if (nwg == 0) return 0;
    dim3 grid((unsigned)nwg);
    const bool slip = a.use_slip != 0, skip0 = a.skip_pen == 0.0f, dv = f.out_div != 1.0f || f.in_div != 1.0f;
    if (!a.use_slip && !single) {
        const size_t ldt = (size_t)SH_FVT_LDS_FLOATS * 4;
        static const bool keep_clamp = getenv("SH_FVT_KEEP_CLAMP") != nullptr;      /* (A/B switch) */
        const bool nc = f.no_clamp && !dv && !keep_clamp;
        return pick_bool([&](auto sk, auto d, auto n) {
            if constexpr (d() && n()) return -1;      /* never reached, nc implies !dv: the family has six forms of eight, and these two are not instantiated */
            else return launch_k<k_ff_viterbi_teams<sk(), d(), n()>>(grid, dim3(SH_FVT_NTH), ldt, s, f, a, md);
        }, skip0, dv, nc);
    }
    return pick_bool([&](auto sl, auto sk, auto d) { return launch_k<k_ff_viterbi<sl(), sk(), d()>>(grid, dim3(512), lds, s, f, a, md); }, slip, skip0, dv);
}
