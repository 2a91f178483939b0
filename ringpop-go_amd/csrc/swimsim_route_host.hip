// swimsim_route_host.hip — the host side of key routing and replica sets: swimsim_route, swimsim_route_census,
// swimsim_route_n and swimsim_replica_census (kernels: swimsim_route.hip), of forwarded requests:
// swimsim_forward and swimsim_forward_census (kernels: swimsim_forward.hip), and of the ring
// checksums: swimsim_ring_checksums and swimsim_ring_census (kernels: swimsim_ringcs.hip). Part of
// swimsim_engine.hip, which includes it after struct swimsim and the helpers it uses (dalloc, stream_sync, DeviceScope).

// ---- key routing through the observers' ring views (swimsim_route.hip) ----
namespace {

constexpr size_t ROUTE_OWN_WORDS = (size_t)16 << 20;     // owners held on the device per launch of swimsim_route (64 MiB)
constexpr size_t ROUTE_EXC_MAX = (size_t)4 << 20;        // exception pairs of a census pass at most (28 B each: 112 MiB)
constexpr size_t ROUTE_EXC_MIN = 65536;
constexpr size_t ROUTE_RUNS_FIRST = 65536;               // runs read back with the run count; more take a second copy

// grow a route scratch buffer to `need` elements (the old content is not kept)
extern "C++" template <typename T>
int route_grow(swimsim *h, T **p, size_t *cap, size_t need, const char *what) {
    if (need <= *cap) return 0;
    if (*p) {
        HIPCHK(h, stream_sync(h));
        dfree(h, p, dalloc_bytes(*cap, sizeof(T)));
        *cap = 0;
    }
    const size_t c = need + need / 2;
    if (int rc = dalloc(h, p, c, what)) return rc;
    *cap = c;
    return 0;
}

// A routing kernel's dynamic LDS is the presence bitmap. Where it and the kernel's static_bytes pass the default 64 KB,
// the dynamic part must be allowed, for the route and the census variant of the kernel
extern "C++" template <typename K>
int route_allow_lds(swimsim *h, size_t static_bytes, K *kernel_a, K *kernel_b) {
    if ((size_t)route_bitmap_bytes(h->NP) + static_bytes > 65536)
        for (K *k : {kernel_a, kernel_b})
            HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)route_bitmap_bytes(h->NP)));
    return 0;
}

// the point table of `R` replica points, built at its first use: hash every (member, replica), sort the points
int route_table(swimsim *h, uint32_t R, const swimsim::RouteTable **out) {
    for (const swimsim::RouteTable &t : h->rt_tabs)
        if (t.R == R) {
            *out = &t;
            return 0;
        }
    const size_t P = (size_t)h->N * R;
    swimsim::RouteTable t{R, nullptr, nullptr};
    unsigned long long *alt = nullptr;
    void *tmp = nullptr;
    size_t tmp_bytes = 0;
    hipcub::DoubleBuffer<unsigned long long> probe(nullptr, nullptr);
    HIPCHK(h, hipcub::DeviceRadixSort::SortKeys(nullptr, tmp_bytes, probe, (int)P, 0, 64, h->s));
    int rc = 0;
    uint8_t *tmp8 = nullptr;
    if ((rc = dalloc(h, &t.hm, P, "route replica hashes")) || (rc = dalloc(h, &t.pts, P, "route points")) ||
        (rc = dalloc(h, &alt, P, "route sort buffer")) || (rc = dalloc(h, &tmp8, tmp_bytes, "route sort scratch"))) {
        dfree(h, &t.hm, dalloc_bytes(P, 4));
        dfree(h, &t.pts, dalloc_bytes(P, 8));
        dfree(h, &alt, dalloc_bytes(P, 8));
        return rc;
    }
    tmp = tmp8;
    hipLaunchKernelGGL(k_route_points, dim3((uint32_t)((P + 255) / 256)), dim3(256), 0, h->s, h->d.addrw, h->W, h->N, R, t.hm,
                       t.pts);
    hipcub::DoubleBuffer<unsigned long long> db(t.pts, alt);
    hipError_t e = hipcub::DeviceRadixSort::SortKeys(tmp, tmp_bytes, db, (int)P, 0, 64, h->s);
    if (e == hipSuccess) e = stream_sync(h);
    if (e == hipSuccess) e = hipGetLastError();
    if (db.Current() != t.pts) std::swap(t.pts, alt);                // (both hold P points: the table keeps the sorted one)
    dfree(h, &alt, dalloc_bytes(P, 8));
    dfree(h, &tmp8, dalloc_bytes(tmp_bytes, 1));
    if (e != hipSuccess) {
        dfree(h, &t.hm, dalloc_bytes(P, 4));
        dfree(h, &t.pts, dalloc_bytes(P, 8));
        return h->fail(SWIMSIM_EHIP, "route point table: %s", hipGetErrorString(e));
    }
    h->rt_tabs.push_back(t);
    *out = &h->rt_tabs.back();
    return 0;
}

// what both entry points refuse before any device work
int route_check(swimsim *h, const uint8_t *keys, const uint64_t *off, size_t nkeys, uint32_t R, int32_t mode, const char *who) {
    if (!keys || !off || nkeys == 0) return h->fail(SWIMSIM_EINVAL, "%s: no keys", who);
    if (nkeys > 0x80000000ull) return h->fail(SWIMSIM_EINVAL, "%s: %zu keys are more than 2^31", who, nkeys);
    if (R < 1 || R > ROUTE_R_MAX) return h->fail(SWIMSIM_EINVAL, "%s: replica_points %u not in 1..%u", who, R, ROUTE_R_MAX);
    if (mode < 0 || mode > 2) return h->fail(SWIMSIM_EINVAL, "%s: unknown mode %d", who, mode);
    if (h->N > ROUTE_N_MAX) return h->fail(SWIMSIM_EINVAL, "%s: %u members are more than %u", who, h->N, ROUTE_N_MAX);
    for (size_t k = 0; k < nkeys; k++)
        if (off[k + 1] < off[k] || off[k + 1] - off[k] > 0xFFFFFFFFull)
            return h->fail(SWIMSIM_EINVAL, "%s: key offsets must ascend", who);
    return 0;
}

// upload the keys, make the point table, hash the keys and find their lower bounds (launches on the main stream)
int route_keys(swimsim *h, const uint8_t *keys, const uint64_t *off, size_t nkeys, uint32_t R, const swimsim::RouteTable **tab) {
    const size_t nb = off[nkeys] - off[0];
    int rc = 0;
    if ((rc = route_grow(h, &h->rt_bytes, &h->rt_bytes_cap, nb + 8, "route key bytes"))) return rc;
    if (nkeys + 1 > h->rt_keys_cap) {
        if (h->rt_off) HIPCHK(h, stream_sync(h));
        dfree(h, &h->rt_off, dalloc_bytes(h->rt_keys_cap, 8));
        dfree(h, &h->rt_kh, dalloc_bytes(h->rt_keys_cap, 4));
        dfree(h, &h->rt_p0, dalloc_bytes(h->rt_keys_cap, 4));
        dfree(h, &h->rt_base, dalloc_bytes(h->rt_keys_cap, 4));
        h->rt_keys_cap = 0;
        const size_t c = nkeys + 1 + nkeys / 2;
        if ((rc = dalloc(h, &h->rt_off, c, "route key offsets")) || (rc = dalloc(h, &h->rt_kh, c, "route key hashes")) ||
            (rc = dalloc(h, &h->rt_p0, c, "route lower bounds")) || (rc = dalloc(h, &h->rt_base, c, "route base owners"))) {
            dfree(h, &h->rt_off, dalloc_bytes(c, 8));
            dfree(h, &h->rt_kh, dalloc_bytes(c, 4));
            dfree(h, &h->rt_p0, dalloc_bytes(c, 4));
            return rc;
        }
        h->rt_keys_cap = c;
    }
    if ((rc = route_table(h, R, tab))) return rc;
    for (hipEvent_t &e : h->rt_ev)
        if (!e) HIPCHK(h, hipEventCreate(&e));
    if ((rc = route_allow_lds(h, 4096, &k_route<false>, &k_route<true>))) return rc;   // (N above ~491,000)
    std::vector<uint64_t> &rel = h->rt_rel;                          // offsets from the first key's byte
    rel.resize(nkeys + 1);
    for (size_t k = 0; k <= nkeys; k++) rel[k] = off[k] - off[0];
    if (nb) HIPCHK(h, hipMemcpyAsync(h->rt_bytes, keys + off[0], nb, hipMemcpyHostToDevice, h->s));
    HIPCHK(h, hipMemsetAsync(h->rt_bytes + nb, 0, 8, h->s));
    HIPCHK(h, hipMemcpyAsync(h->rt_off, rel.data(), (nkeys + 1) * 8, hipMemcpyHostToDevice, h->s));
    HIPCHK(h, hipEventRecord(h->rt_ev[0], h->s));
    hipLaunchKernelGGL(k_route_keys, dim3(blocks_for_threads((uint32_t)nkeys)), dim3(256), 0, h->s, h->rt_bytes, h->rt_off,
                       (uint32_t)nkeys, (*tab)->pts, h->N * R, h->rt_kh, h->rt_p0);
    return 0;
}

// the census scratch, allocated at the first census of the handle: E exception pairs (appended, sorted, run-length encoded
// with counts), the cursor and the hipcub scratch. E is at least `floor`, the most pairs a pass over one key can append
// (NL for swimsim_route_census, 2n * NL for swimsim_replica_census), so that halving the keys of an overflowing pass
// ends; a buffer that is below a later call's floor is replaced.
int route_exc_scratch(swimsim *h, size_t floor) {
    if (h->rt_exc && h->rt_exc_cap >= floor) return 0;
    if (h->rt_exc) {
        HIPCHK(h, stream_sync(h));
        uint8_t *cub8 = static_cast<uint8_t *>(h->rt_cub);
        dfree(h, &h->rt_exc, dalloc_bytes(h->rt_exc_cap, 8));
        dfree(h, &h->rt_exc2, dalloc_bytes(h->rt_exc_cap, 8));
        dfree(h, &h->rt_uniq, dalloc_bytes(h->rt_exc_cap, 8));
        dfree(h, &h->rt_cnt, dalloc_bytes(h->rt_exc_cap, 4));
        dfree(h, &h->rt_cur, dalloc_bytes(2, 8));
        dfree(h, &cub8, dalloc_bytes(h->rt_cub_bytes, 1));
        h->rt_cub = nullptr;
        h->rt_cub_bytes = h->rt_exc_cap = 0;
    }
    size_t E = std::min(ROUTE_EXC_MAX, std::max(ROUTE_EXC_MIN, (size_t)h->NL * 64));
    if (const char *v = getenv("SWIMSIM_ROUTE_EXC_CAP")) E = (size_t)strtoull(v, nullptr, 10);   // (tests: the chunked passes)
    E = std::min<size_t>(std::max<size_t>(E, floor), (size_t)1 << 30);
    size_t b1 = 0, b2 = 0;
    hipcub::DoubleBuffer<unsigned long long> probe(nullptr, nullptr);
    HIPCHK(h, hipcub::DeviceRadixSort::SortKeys(nullptr, b1, probe, (int)E, 0, 64, h->s));
    HIPCHK(h, hipcub::DeviceRunLengthEncode::Encode(nullptr, b2, (unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                                   (uint32_t *)nullptr, (uint32_t *)nullptr, (int)E, h->s));
    const size_t cb = std::max(b1, b2);
    uint8_t *cub8 = nullptr;
    int rc = 0;
    if ((rc = dalloc(h, &h->rt_exc, E, "route exception pairs")) || (rc = dalloc(h, &h->rt_exc2, E, "route sorted pairs")) ||
        (rc = dalloc(h, &h->rt_uniq, E, "route runs")) || (rc = dalloc(h, &h->rt_cnt, E, "route run counts")) ||
        (rc = dalloc(h, &h->rt_cur, 2, "route cursor")) || (rc = dalloc(h, &cub8, cb, "route sort scratch"))) {
        dfree(h, &h->rt_exc, dalloc_bytes(E, 8));
        dfree(h, &h->rt_exc2, dalloc_bytes(E, 8));
        dfree(h, &h->rt_uniq, dalloc_bytes(E, 8));
        dfree(h, &h->rt_cnt, dalloc_bytes(E, 4));
        dfree(h, &h->rt_cur, dalloc_bytes(2, 8));
        return rc;
    }
    h->rt_cub = cub8;
    h->rt_cub_bytes = cb;
    h->rt_exc_cap = E;
    return 0;
}

RouteArgs route_args(swimsim *h, const swimsim::RouteTable *tab, size_t nkeys, int32_t mode) {
    RouteArgs a{};
    a.pts = tab->pts; a.hm = tab->hm; a.P = h->N * tab->R; a.R = tab->R;
    a.kh = h->rt_kh; a.p0 = h->rt_p0; a.k0 = 0; a.k1 = (uint32_t)nkeys; a.K = (uint32_t)nkeys;
    a.mode = (uint32_t)mode;
    return a;
}

// ---- the two calls that answer for listed observers (swimsim_route, swimsim_route_n) ----

// The observers of such a call must be rows of this handle. *rows = their local rows, for which rt_rows is grown;
// route_rows uploads them, inside the timed interval, so the vector lives in the caller until the call returns.
int route_observers(swimsim *h, const uint32_t *observers, size_t nobs, const char *what, std::vector<uint32_t> *rows) {
    if (!observers || nobs == 0) return h->fail(SWIMSIM_EINVAL, "%s: no observers", what);
    for (size_t j = 0; j < nobs; j++)
        if (observers[j] < h->lo || observers[j] >= h->lo + h->NL)
            return h->fail(SWIMSIM_EINVAL, "%s: observer %u is not a row of this handle", what, observers[j]);
    if (nobs > 0xFFFFFFFFull) return h->fail(SWIMSIM_EINVAL, "%s: list of %zu observers too long", what, nobs);
    if (int rc = route_grow(h, &h->rt_rows, &h->rt_rows_cap, nobs, "route rows")) return rc;
    rows->resize(nobs);
    for (size_t j = 0; j < nobs; j++) (*rows)[j] = observers[j] - h->lo;
    return 0;
}

// The rows of such a call (route_observers), uploaded and then routed `per` per launch: launch(j0, nr) enqueues the
// kernel for rows [j0, j0 + nr), and its result, `words` words per row in rt_own, is copied to out. The timed interval
// (opened by route_keys) closes after the last launch. tail() enqueues what else the caller reads back, before the one
// synchronisation of the call.
extern "C++" template <typename Launch, typename Tail>
int route_rows(swimsim *h, const std::vector<uint32_t> &rows, size_t per, size_t words, int32_t *out, Launch launch, Tail tail,
               double *ms) {
    const size_t nobs = rows.size();
    HIPCHK(h, hipMemcpyAsync(h->rt_rows, rows.data(), nobs * 4, hipMemcpyHostToDevice, h->s));
    for (size_t j0 = 0; j0 < nobs; j0 += per) {
        const size_t nr = std::min(per, nobs - j0);
        launch(j0, nr);
        if (j0 + per >= nobs) HIPCHK(h, hipEventRecord(h->rt_ev[1], h->s));
        HIPCHK(h, hipMemcpyAsync(out + j0 * words, h->rt_own, nr * words * 4, hipMemcpyDeviceToHost, h->s));
    }
    if (int rc = tail()) return rc;
    HIPCHK(h, stream_sync(h));
    HIPCHK(h, hipGetLastError());
    if (ms) {
        float t = 0;
        HIPCHK(h, hipEventElapsedTime(&t, h->rt_ev[0], h->rt_ev[1]));
        *ms = t;
    }
    return SWIMSIM_OK;
}

// ---- the two censuses (swimsim_route_census, swimsim_replica_census) ----

// The counted rows: every row of the handle or its live ones (the host keeps the live table the device holds:
// swimsim_set_live, the events). *first is the first of them, the base row; *counted their number. When no row counts
// the outputs are complete here (no entry for any key) and the caller returns.
int route_counted(swimsim *h, int32_t who, const char *what, size_t nkeys, uint32_t *all, uint32_t *first, uint32_t *counted,
                  uint64_t *hist_off, size_t *nhist, double *ms) {
    if (who != SWIMSIM_CENSUS_LIVE && who != SWIMSIM_CENSUS_ALL) return h->fail(SWIMSIM_EINVAL, "%s: unknown who %d", what, who);
    *all = who == SWIMSIM_CENSUS_ALL;
    *first = SRC_NONE;
    uint32_t ncount = 0;
    for (uint32_t r = 0; r < h->NL; r++)
        if (*all || h->live[h->lo + r]) {
            if (*first == SRC_NONE) *first = r;
            ncount++;
        }
    *counted = ncount;
    *nhist = 0;
    if (ms) *ms = 0;
    if (ncount == 0)
        for (size_t k = 0; k <= nkeys; k++) hist_off[k] = 0;
    return 0;
}

// the census fields of a kernel's arguments: every row but the base row appends its exceptions to the pair buffer
void route_census_args(swimsim *h, RouteArgs *a, uint32_t first, uint32_t all) {
    a->rows = nullptr;
    a->skip_row = first;
    a->all = all;
    a->exc = h->rt_exc;
    a->cursor = h->rt_cur;
    a->exc_cap = h->rt_exc_cap;
}

// The passes of a census over chunks of keys, all keys at first. launch(k0, k1) enqueues the caller's census kernel for
// keys [k0, k1). A pass whose pairs overflow the buffer is run again over half as many keys: nothing of it is used
// (one_key_error(pairs) is the failure of a pass over ONE key, which the floor of route_exc_scratch excludes). The pairs of
// a pass that fits are sorted and run-length encoded, and for every key k of the pass emit(k, runs, rcnt, i0, i1, put)
// turns its runs [i0, i1) (ascending) into histogram entries through put(member, count), which writes the first cap
// entries and counts all of them. The first pass's time includes the keys and the base, which the caller has enqueued.
// first_chunk (0: all keys) bounds the keys of a pass from the start, for a caller whose pass has scratch per key.
extern "C++" template <typename Launch, typename Emit, typename OneKeyError>
int route_census_passes(swimsim *h, size_t nkeys, Launch launch, Emit emit, OneKeyError one_key_error, uint64_t *hist_off,
                        int32_t *hist_member, uint32_t *hist_count, size_t cap, size_t *nhist, double *ms,
                        size_t first_chunk = 0) {
    double total_ms = 0;
    float t = 0;
    uint32_t *nruns_d = reinterpret_cast<uint32_t *>(h->rt_cur + 1);
    std::vector<unsigned long long> runs;
    std::vector<uint32_t> rcnt;
    size_t total = 0, kb = 0, chunk = first_chunk ? std::min(first_chunk, nkeys) : nkeys;
    bool first_pass = true;
    auto put = [&](int32_t member, uint32_t c) {
        if (total < cap) {
            hist_member[total] = member;
            hist_count[total] = c;
        }
        total++;
    };
    while (kb < nkeys) {
        const size_t ke = std::min(nkeys, kb + chunk);
        HIPCHK(h, hipMemsetAsync(h->rt_cur, 0, 16, h->s));
        if (!first_pass) HIPCHK(h, hipEventRecord(h->rt_ev[0], h->s));
        launch((uint32_t)kb, (uint32_t)ke);
        HIPCHK(h, hipEventRecord(h->rt_ev[1], h->s));
        unsigned long long cur = 0;
        HIPCHK(h, hipMemcpyAsync(&cur, h->rt_cur, 8, hipMemcpyDeviceToHost, h->s));
        HIPCHK(h, stream_sync(h));                                   // the pass's host synchronisation
        HIPCHK(h, hipGetLastError());
        first_pass = false;
        HIPCHK(h, hipEventElapsedTime(&t, h->rt_ev[0], h->rt_ev[1]));
        total_ms += t;
        if (cur > h->rt_exc_cap) {                                   // the buffer was full: nothing of this pass is used
            if (ke - kb == 1) return one_key_error(cur);
            chunk = std::max<size_t>(1, (ke - kb) / 2);
            continue;
        }
        size_t nr = 0;
        if (cur) {                                                   // sort the pairs, count the runs of equal pairs
            HIPCHK(h, hipEventRecord(h->rt_ev[0], h->s));
            hipcub::DoubleBuffer<unsigned long long> db(h->rt_exc, h->rt_exc2);
            HIPCHK(h, hipcub::DeviceRadixSort::SortKeys(h->rt_cub, h->rt_cub_bytes, db, (int)cur, 0, 64, h->s));
            HIPCHK(h, hipcub::DeviceRunLengthEncode::Encode(h->rt_cub, h->rt_cub_bytes, db.Current(), h->rt_uniq, h->rt_cnt, nruns_d,
                                                           (int)cur, h->s));
            HIPCHK(h, hipEventRecord(h->rt_ev[1], h->s));
            uint32_t nruns = 0;
            const size_t spec = std::min<size_t>(cur, ROUTE_RUNS_FIRST);
            runs.resize(spec);
            rcnt.resize(spec);
            HIPCHK(h, hipMemcpyAsync(&nruns, nruns_d, 4, hipMemcpyDeviceToHost, h->s));
            HIPCHK(h, hipMemcpyAsync(runs.data(), h->rt_uniq, spec * 8, hipMemcpyDeviceToHost, h->s));
            HIPCHK(h, hipMemcpyAsync(rcnt.data(), h->rt_cnt, spec * 4, hipMemcpyDeviceToHost, h->s));
            HIPCHK(h, stream_sync(h));
            HIPCHK(h, hipEventElapsedTime(&t, h->rt_ev[0], h->rt_ev[1]));
            total_ms += t;
            nr = nruns;
            if (nr > spec) {
                runs.resize(nr);
                rcnt.resize(nr);
                HIPCHK(h, hipMemcpyAsync(runs.data() + spec, h->rt_uniq + spec, (nr - spec) * 8, hipMemcpyDeviceToHost, h->s));
                HIPCHK(h, hipMemcpyAsync(rcnt.data() + spec, h->rt_cnt + spec, (nr - spec) * 4, hipMemcpyDeviceToHost, h->s));
                HIPCHK(h, stream_sync(h));
            }
        }
        // the histogram of keys [kb, ke): the key is the high word of a run, so a key's runs are contiguous
        size_t i = 0;
        for (size_t k = kb; k < ke; k++) {
            hist_off[k] = total;
            const size_t i0 = i;
            while (i < nr && (runs[i] >> 32) == k) i++;
            emit(k, runs, rcnt, i0, i, put);
        }
        kb = ke;
    }
    hist_off[nkeys] = total;
    *nhist = total;
    if (ms) *ms = total_ms;
    return SWIMSIM_OK;
}

// The emit of a census whose pairs are key << 32 | answer + 1, one answer (an owner, a handler; -1: none) per counted
// row and key: the runs of key k are ascending by answer + 1, and base[k], the answer under the first counted row,
// takes the rows that no run counts.
extern "C++" inline auto route_emit_answers(const std::vector<int32_t> &base, uint32_t ncount) {
    return [&base, ncount](size_t k, const std::vector<unsigned long long> &runs, const std::vector<uint32_t> &rcnt, size_t i0,
                           size_t i1, auto put) {
        uint64_t exc = 0;
        for (size_t j = i0; j < i1; j++) exc += rcnt[j];
        const uint32_t bo = (uint32_t)(base[k] + 1), bc = (uint32_t)(ncount - exc);
        bool placed = bc == 0;
        for (size_t i = i0; i < i1; i++) {
            const uint32_t o1 = (uint32_t)runs[i];
            if (!placed && bo < o1) {
                put(base[k], bc);
                placed = true;
            }
            put((int32_t)o1 - 1, rcnt[i]);
        }
        if (!placed) put(base[k], bc);
    };
}

}  // namespace

int swimsim_route(swimsim_t *h, const uint8_t *keys, const uint64_t *off, size_t nkeys, uint32_t replica_points,
                  const uint32_t *observers, size_t nobs, int32_t mode, int32_t *owners, double *ms) {
    if (!h) return SWIMSIM_EINVAL;
    if (!owners) return h->fail(SWIMSIM_EINVAL, "route: no output buffer");
    if (int rc = route_check(h, keys, off, nkeys, replica_points, mode, "route")) return rc;
    DeviceScope ds(h->device);
    std::vector<uint32_t> rows;
    const swimsim::RouteTable *tab = nullptr;
    const size_t per = std::max<size_t>(1, std::min(nobs, ROUTE_OWN_WORDS / nkeys));   // rows per launch
    int rc = 0;
    if ((rc = route_observers(h, observers, nobs, "route", &rows)) ||
        (rc = route_grow(h, &h->rt_own, &h->rt_own_cap, per * nkeys, "route owners")) ||
        (rc = route_keys(h, keys, off, nkeys, replica_points, &tab)))
        return rc;
    RouteArgs a = route_args(h, tab, nkeys, mode);
    a.owners = h->rt_own;
    auto launch = [&](size_t j0, size_t nr) {
        a.rows = h->rt_rows + j0;
        hipLaunchKernelGGL(k_route<false>, dim3((uint32_t)nr), dim3(ROUTE_THREADS), route_bitmap_bytes(h->NP), h->s, h->d, a);
    };
    return route_rows(h, rows, per, nkeys, owners, launch, [] { return 0; }, ms);
}

int swimsim_route_census(swimsim_t *h, const uint8_t *keys, const uint64_t *off, size_t nkeys, uint32_t replica_points,
                         int32_t who, int32_t mode, uint32_t *counted, uint64_t *hist_off, int32_t *hist_owner,
                         uint32_t *hist_count, size_t cap, size_t *nhist, double *ms) {
    if (!h) return SWIMSIM_EINVAL;
    if (!counted || !hist_off || !nhist || (cap && (!hist_owner || !hist_count)))
        return h->fail(SWIMSIM_EINVAL, "route census: no output buffer");
    if (int rc = route_check(h, keys, off, nkeys, replica_points, mode, "route census")) return rc;
    uint32_t all = 0, first = SRC_NONE;
    if (int rc = route_counted(h, who, "route census", nkeys, &all, &first, counted, hist_off, nhist, ms)) return rc;
    const uint32_t ncount = *counted;
    if (ncount == 0) return SWIMSIM_OK;
    DeviceScope ds(h->device);
    // scratch, on first use: the exception pairs of one pass. A pass over one key appends at most NL pairs, so a
    // buffer of at least NL pairs always ends the chunking
    if (int rc = route_exc_scratch(h, h->NL)) return rc;
    const swimsim::RouteTable *tab = nullptr;
    int rc = 0;
    if ((rc = route_grow(h, &h->rt_rows, &h->rt_rows_cap, 1, "route rows"))) return rc;
    if ((rc = route_keys(h, keys, off, nkeys, replica_points, &tab))) return rc;
    // base[k]: the owner under the first counted row
    HIPCHK(h, hipMemcpyAsync(h->rt_rows, &first, 4, hipMemcpyHostToDevice, h->s));
    RouteArgs a = route_args(h, tab, nkeys, mode);
    a.rows = h->rt_rows;
    a.owners = h->rt_base;
    hipLaunchKernelGGL(k_route<false>, dim3(1), dim3(ROUTE_THREADS), route_bitmap_bytes(h->NP), h->s, h->d, a);
    std::vector<int32_t> base(nkeys);
    HIPCHK(h, hipMemcpyAsync(base.data(), h->rt_base, nkeys * 4, hipMemcpyDeviceToHost, h->s));
    a.owners = nullptr;
    a.base = h->rt_base;
    route_census_args(h, &a, first, all);
    auto launch = [&](uint32_t k0, uint32_t k1) {
        a.k0 = k0;
        a.k1 = k1;
        hipLaunchKernelGGL(k_route<true>, dim3(h->NL), dim3(ROUTE_THREADS), route_bitmap_bytes(h->NP), h->s, h->d, a);
    };
    auto one_key_error = [&](unsigned long long cur) {
        return h->fail(SWIMSIM_EHIP, "route census: %llu exceptions of one key over %u rows", cur, h->NL);
    };
    return route_census_passes(h, nkeys, launch, route_emit_answers(base, ncount), one_key_error, hist_off, hist_owner,
                               hist_count, cap, nhist, ms);
}

// ---- replica sets through the observers' ring views (k_route_n) ----
namespace {

int route_n_check(swimsim *h, uint32_t n, const char *who) {
    if (n < 1 || n > ROUTE_NN_MAX) return h->fail(SWIMSIM_EINVAL, "%s: n %u not in 1..%u", who, n, ROUTE_NN_MAX);
    return 0;
}

}  // namespace

int swimsim_route_n(swimsim_t *h, const uint8_t *keys, const uint64_t *off, size_t nkeys, uint32_t replica_points, uint32_t n,
                    const uint32_t *observers, size_t nobs, int32_t mode, int32_t *prefs, uint32_t *servers, double *ms) {
    if (!h) return SWIMSIM_EINVAL;
    if (!prefs) return h->fail(SWIMSIM_EINVAL, "route_n: no output buffer");
    if (int rc = route_check(h, keys, off, nkeys, replica_points, mode, "route_n")) return rc;
    if (int rc = route_n_check(h, n, "route_n")) return rc;
    DeviceScope ds(h->device);
    std::vector<uint32_t> rows;
    const swimsim::RouteTable *tab = nullptr;
    const size_t per_key = nkeys * n;                                // words of one row's lists
    const size_t per = std::max<size_t>(1, std::min(nobs, ROUTE_OWN_WORDS / per_key));   // rows per launch
    int rc = 0;
    if ((rc = route_observers(h, observers, nobs, "route_n", &rows)) ||
        (rc = route_grow(h, &h->rt_srv, &h->rt_srv_cap, nobs, "route server counts")) ||
        (rc = route_grow(h, &h->rt_own, &h->rt_own_cap, per * per_key, "route owners")) ||
        (rc = route_keys(h, keys, off, nkeys, replica_points, &tab)) ||
        (rc = route_allow_lds(h, ROUTE_N_STATIC_LDS, &k_route_n<false>, &k_route_n<true>)))
        return rc;
    RouteNArgs a{};
    a.r = route_args(h, tab, nkeys, mode);
    a.n = n;
    a.prefs = h->rt_own;
    auto launch = [&](size_t j0, size_t nr) {
        a.r.rows = h->rt_rows + j0;
        a.servers = h->rt_srv + j0;
        hipLaunchKernelGGL(k_route_n<false>, dim3((uint32_t)nr), dim3(ROUTE_THREADS), route_bitmap_bytes(h->NP), h->s, h->d, a);
    };
    auto tail = [&] {
        if (servers) HIPCHK(h, hipMemcpyAsync(servers, h->rt_srv, nobs * 4, hipMemcpyDeviceToHost, h->s));
        return 0;
    };
    return route_rows(h, rows, per, per_key, prefs, launch, tail, ms);
}

int swimsim_replica_census(swimsim_t *h, const uint8_t *keys, const uint64_t *off, size_t nkeys, uint32_t replica_points, uint32_t n,
                           int32_t who, int32_t mode, uint32_t *counted, uint64_t *hist_off, int32_t *hist_member,
                           uint32_t *hist_count, size_t cap, size_t *nhist, double *ms) {
    if (!h) return SWIMSIM_EINVAL;
    if (!counted || !hist_off || !nhist || (cap && (!hist_member || !hist_count)))
        return h->fail(SWIMSIM_EINVAL, "replica census: no output buffer");
    if (int rc = route_check(h, keys, off, nkeys, replica_points, mode, "replica census")) return rc;
    if (int rc = route_n_check(h, n, "replica census")) return rc;
    uint32_t all = 0, first = SRC_NONE;
    if (int rc = route_counted(h, who, "replica census", nkeys, &all, &first, counted, hist_off, nhist, ms)) return rc;
    const uint32_t ncount = *counted;
    if (ncount == 0) return SWIMSIM_OK;
    DeviceScope ds(h->device);
    // A row appends, per key, at most n members its set has beyond the base and n the base has beyond its set: a pass
    // over one key appends at most 2n * NL pairs, so a buffer of at least 2n * NL pairs always ends the chunking
    int rc = 0;
    if ((rc = route_exc_scratch(h, (size_t)2 * n * h->NL))) return rc;
    const swimsim::RouteTable *tab = nullptr;
    if ((rc = route_grow(h, &h->rt_rows, &h->rt_rows_cap, 1, "route rows")) ||
        (rc = route_grow(h, &h->rt_nbase, &h->rt_nbase_cap, nkeys * n, "route base sets")))
        return rc;
    if ((rc = route_keys(h, keys, off, nkeys, replica_points, &tab)) ||
        (rc = route_allow_lds(h, ROUTE_N_STATIC_LDS, &k_route_n<false>, &k_route_n<true>)))
        return rc;
    // nbase[k][*]: the set under the first counted row
    HIPCHK(h, hipMemcpyAsync(h->rt_rows, &first, 4, hipMemcpyHostToDevice, h->s));
    RouteNArgs a{};
    a.r = route_args(h, tab, nkeys, mode);
    a.n = n;
    a.r.rows = h->rt_rows;
    a.prefs = h->rt_nbase;
    hipLaunchKernelGGL(k_route_n<false>, dim3(1), dim3(ROUTE_THREADS), route_bitmap_bytes(h->NP), h->s, h->d, a);
    std::vector<int32_t> base(nkeys * n);
    HIPCHK(h, hipMemcpyAsync(base.data(), h->rt_nbase, nkeys * n * 4, hipMemcpyDeviceToHost, h->s));
    a.prefs = nullptr;
    a.nbase = h->rt_nbase;
    route_census_args(h, &a.r, first, all);
    auto launch = [&](uint32_t k0, uint32_t k1) {
        a.r.k0 = k0;
        a.r.k1 = k1;
        hipLaunchKernelGGL(k_route_n<true>, dim3(h->NL), dim3(ROUTE_THREADS), route_bitmap_bytes(h->NP), h->s, h->d, a);
    };
    // the runs of key k are ascending by (member, sign). A base member is listed by every counted row but those of its
    // sign-1 run; any other member by the rows of its sign-0 run. Zero counts are omitted
    auto emit = [&](size_t k, const std::vector<unsigned long long> &runs, const std::vector<uint32_t> &rcnt, size_t i0, size_t i1,
                    auto put) {
        auto some = [&](int32_t member, uint32_t c) {
            if (c) put(member, c);
        };
        int32_t bs[ROUTE_NN_MAX];
        uint32_t nb = 0, bi = 0;
        for (uint32_t j = 0; j < n && base[k * n + j] >= 0; j++) bs[nb++] = base[k * n + j];
        std::sort(bs, bs + nb);
        for (size_t i = i0; i < i1; i++) {
            const int32_t m = (int32_t)(((uint32_t)runs[i]) >> 1) - 1;
            while (bi < nb && bs[bi] < m) some(bs[bi++], ncount);
            if (bi < nb && bs[bi] == m) {                            // (its run has sign 1)
                some(m, ncount - rcnt[i]);
                bi++;
            } else {
                some(m, rcnt[i]);
            }
        }
        while (bi < nb) some(bs[bi++], ncount);
    };
    auto one_key_error = [&](unsigned long long cur) {
        return h->fail(SWIMSIM_EHIP, "replica census: %llu exceptions of one key over %u rows, n = %u", cur, h->NL, n);
    };
    return route_census_passes(h, nkeys, launch, emit, one_key_error, hist_off, hist_member, hist_count, cap, nhist, ms);
}

// ---- requests forwarded through the observers' ring views (swimsim_forward.hip) ----
namespace {

constexpr size_t FWD_OWN_WORDS = (size_t)64 << 20;       // the owner table of one pass at most (256 MiB): 1,024 keys at 65,536 rows
constexpr size_t FWD_REQ_SLICE = (size_t)4 << 20;        // requests of one listed launch at most (22 B each on the device)
constexpr size_t FWD_TEST_CHUNK = 8;                     // mode 3 (tests): keys per pass

// the HIP events of a call's passes, three per pass (before the table, after it, after the chases); destroyed with the call
struct FwdEvents {
    std::vector<hipEvent_t> ev;
    ~FwdEvents() {
        for (hipEvent_t e : ev) hipEventDestroy(e);
    }
    hipError_t mark(hipStream_t s) {
        hipEvent_t e = nullptr;
        hipError_t rc = hipEventCreate(&e);
        if (rc != hipSuccess) return rc;
        ev.push_back(e);
        return hipEventRecord(e, s);
    }
    // after the stream is synchronised: the passes' table and chase times
    hipError_t split(double *table_ms, double *chase_ms) const {
        *table_ms = *chase_ms = 0;
        for (size_t i = 0; i + 2 < ev.size(); i += 3) {
            float a = 0, b = 0;
            hipError_t rc = hipEventElapsedTime(&a, ev[i], ev[i + 1]);
            if (rc == hipSuccess) rc = hipEventElapsedTime(&b, ev[i + 1], ev[i + 2]);
            if (rc != hipSuccess) return rc;
            *table_ms += a;
            *chase_ms += b;
        }
        return hipSuccess;
    }
};

// what both entry points refuse before any device work, beyond the output pointers; *chunk = the keys of a pass
int fwd_check(swimsim *h, const uint8_t *keys, const uint64_t *off, size_t nkeys, uint32_t R, uint32_t max_hops, int32_t policy,
              int32_t mode, const char *who, size_t *chunk) {
    if (mode < 0 || mode > 3) return h->fail(SWIMSIM_EINVAL, "%s: unknown mode %d", who, mode);
    if (int rc = route_check(h, keys, off, nkeys, R, mode == 3 ? 0 : mode, who)) return rc;
    if (max_hops < 1 || max_hops > FWD_HOPS_MAX) return h->fail(SWIMSIM_EINVAL, "%s: max_hops %u not in 1..%u", who, max_hops, FWD_HOPS_MAX);
    if (policy != SWIMSIM_FWD_CHAIN && policy != SWIMSIM_FWD_ONE_HOP) return h->fail(SWIMSIM_EINVAL, "%s: unknown policy %d", who, policy);
    if (h->NL != h->N)
        return h->fail(SWIMSIM_EINVAL, "%s: this handle holds rows %u..%u of %u; a chain may visit any row, and chains that cross "
                       "shards are not supported", who, h->lo, h->lo + h->NL, h->N);
    *chunk = std::min(nkeys, mode == 3 ? FWD_TEST_CHUNK : std::max<size_t>(1, FWD_OWN_WORDS / h->N));
    return 0;
}

// the owner table of `chunk` keys, on first use (exactly chunk * N words: the table is the call's largest buffer)
int fwd_table_scratch(swimsim *h, size_t chunk) {
    const size_t need = chunk * h->N;
    if (need > h->fw_own_cap) {
        if (h->fw_own) HIPCHK(h, stream_sync(h));
        dfree(h, &h->fw_own, dalloc_bytes(h->fw_own_cap, 4));
        h->fw_own_cap = 0;
        if (int rc = dalloc(h, &h->fw_own, need, "forward owner table")) return rc;
        h->fw_own_cap = need;
    }
    return route_allow_lds(h, 4096, &k_fwd_table, &k_fwd_table);     // (N above ~491,000)
}

// the table of keys [k0, k1): own[(k - k0) * N + row] for every live row
void fwd_table(swimsim *h, const swimsim::RouteTable *tab, size_t nkeys, int32_t mode, uint32_t k0, uint32_t k1) {
    RouteArgs a = route_args(h, tab, nkeys, mode == 3 ? 0 : mode);
    a.k0 = k0;
    a.k1 = k1;
    a.owners = h->fw_own;
    hipLaunchKernelGGL(k_fwd_table, dim3(h->N), dim3(ROUTE_THREADS), route_bitmap_bytes(h->NP), h->s, h->d, a);
}

FwdArgs fwd_args(swimsim *h, uint32_t k0, uint32_t k1, uint32_t max_hops, int32_t policy) {
    FwdArgs f{};
    f.own = h->fw_own;
    f.k0 = k0; f.k1 = k1;
    f.max_hops = max_hops;
    f.one_hop = policy == SWIMSIM_FWD_ONE_HOP;
    return f;
}

}  // namespace

int swimsim_forward(swimsim_t *h, const uint8_t *keys, const uint64_t *off, size_t nkeys, uint32_t replica_points,
                    const uint32_t *entry, const uint32_t *key_index, size_t nreq, uint32_t max_hops, int32_t policy, int32_t mode,
                    uint8_t *outcome, uint8_t *hops, int32_t *handler, int32_t *holder, int32_t *next, double *ms) {
    if (!h) return SWIMSIM_EINVAL;
    if (!outcome || !hops) return h->fail(SWIMSIM_EINVAL, "forward: no output buffer");
    size_t chunk = 0;
    if (int rc = fwd_check(h, keys, off, nkeys, replica_points, max_hops, policy, mode, "forward", &chunk)) return rc;
    if (!entry || nreq == 0) return h->fail(SWIMSIM_EINVAL, "forward: no requests");
    if (!key_index && nreq % nkeys) return h->fail(SWIMSIM_EINVAL, "forward: %zu requests are no multiple of %zu keys", nreq, nkeys);
    const size_t nent = key_index ? nreq : nreq / nkeys;             // the entries listed
    for (size_t i = 0; i < nent; i++)
        if (entry[i] >= h->N) return h->fail(SWIMSIM_EINVAL, "forward: entry node %u out of range", entry[i]);
    // the requests in key order, so that a pass finds its own in one piece and a wave's lanes share a column:
    // start[k] = the first request of key k; with key_index, order[] lists the requests (stable within a key)
    std::vector<uint64_t> start(nkeys + 1, 0);
    std::vector<uint32_t> sent, skey;
    std::vector<size_t> order;
    if (key_index) {
        for (size_t i = 0; i < nreq; i++) {
            if (key_index[i] >= nkeys) return h->fail(SWIMSIM_EINVAL, "forward: key index %u out of range", key_index[i]);
            start[key_index[i] + 1]++;
        }
        for (size_t k = 0; k < nkeys; k++) start[k + 1] += start[k];
        std::vector<uint64_t> at(start.begin(), start.end() - 1);
        order.resize(nreq); sent.resize(nreq); skey.resize(nreq);
        for (size_t i = 0; i < nreq; i++) {
            const size_t p = at[key_index[i]]++;
            order[p] = i; sent[p] = entry[i]; skey[p] = key_index[i];
        }
    } else {
        for (size_t k = 0; k <= nkeys; k++) start[k] = (uint64_t)k * nent;
    }
    DeviceScope ds(h->device);
    const size_t slice = std::min(nreq, FWD_REQ_SLICE);
    const swimsim::RouteTable *tab = nullptr;
    int rc = 0;
    if ((rc = fwd_table_scratch(h, chunk)) ||
        (rc = route_grow(h, &h->fw_ent, &h->fw_ent_cap, key_index ? slice : nent, "forward entries")))
        return rc;
    if (slice > h->fw_req_cap) {                                     // the requests' keys and outputs, one capacity
        if (h->fw_key) HIPCHK(h, stream_sync(h));
        const size_t o = h->fw_req_cap;
        auto drop = [&](size_t c) {
            dfree(h, &h->fw_key, dalloc_bytes(c, 4));
            dfree(h, &h->fw_outcome, dalloc_bytes(c, 1));
            dfree(h, &h->fw_hops, dalloc_bytes(c, 1));
            dfree(h, &h->fw_handler, dalloc_bytes(c, 4));
            dfree(h, &h->fw_holder, dalloc_bytes(c, 4));
            dfree(h, &h->fw_next, dalloc_bytes(c, 4));
        };
        drop(o);
        h->fw_req_cap = 0;
        const size_t c = std::min(FWD_REQ_SLICE, slice + slice / 2);
        if ((rc = dalloc(h, &h->fw_key, c, "forward key indices")) || (rc = dalloc(h, &h->fw_outcome, c, "forward outcomes")) ||
            (rc = dalloc(h, &h->fw_hops, c, "forward hops")) || (rc = dalloc(h, &h->fw_handler, c, "forward handlers")) ||
            (rc = dalloc(h, &h->fw_holder, c, "forward holders")) || (rc = dalloc(h, &h->fw_next, c, "forward destinations"))) {
            drop(c);                                                 // (a buffer that was not allocated is skipped)
            return rc;
        }
        h->fw_req_cap = c;
    }
    if ((rc = route_keys(h, keys, off, nkeys, replica_points, &tab))) return rc;
    if (!key_index) HIPCHK(h, hipMemcpyAsync(h->fw_ent, entry, nent * 4, hipMemcpyHostToDevice, h->s));
    // the outputs in key order; they reach the caller's buffers only when the call has succeeded
    std::vector<uint8_t> o_out(nreq), o_hops(nreq);
    std::vector<int32_t> o_handler(handler ? nreq : 0), o_holder(holder ? nreq : 0), o_next(next ? nreq : 0);
    FwdEvents evs;
    for (size_t kb = 0; kb < nkeys; kb += chunk) {
        const size_t ke = std::min(nkeys, kb + chunk);
        HIPCHK(h, evs.mark(h->s));
        fwd_table(h, tab, nkeys, mode, (uint32_t)kb, (uint32_t)ke);
        HIPCHK(h, evs.mark(h->s));
        FwdArgs f = fwd_args(h, (uint32_t)kb, (uint32_t)ke, max_hops, policy);
        f.ent = h->fw_ent;
        f.key = key_index ? h->fw_key : nullptr;
        f.nent = (uint32_t)nent;
        f.outcome = h->fw_outcome; f.hops = h->fw_hops;
        f.handler = h->fw_handler; f.holder = h->fw_holder; f.next = h->fw_next;
        for (uint64_t r0 = start[kb]; r0 < start[ke]; r0 += slice) {
            const size_t nr = (size_t)std::min<uint64_t>(slice, start[ke] - r0);
            if (key_index) {
                HIPCHK(h, hipMemcpyAsync(h->fw_ent, sent.data() + r0, nr * 4, hipMemcpyHostToDevice, h->s));
                HIPCHK(h, hipMemcpyAsync(h->fw_key, skey.data() + r0, nr * 4, hipMemcpyHostToDevice, h->s));
            }
            f.at = r0 - start[kb];
            f.nreq = (uint32_t)nr;
            hipLaunchKernelGGL(k_fwd_chase<false>, dim3(blocks_for_threads((uint32_t)nr)), dim3(FWD_THREADS), 0, h->s, h->d, f);
            HIPCHK(h, hipMemcpyAsync(o_out.data() + r0, h->fw_outcome, nr, hipMemcpyDeviceToHost, h->s));
            HIPCHK(h, hipMemcpyAsync(o_hops.data() + r0, h->fw_hops, nr, hipMemcpyDeviceToHost, h->s));
            if (handler) HIPCHK(h, hipMemcpyAsync(o_handler.data() + r0, h->fw_handler, nr * 4, hipMemcpyDeviceToHost, h->s));
            if (holder) HIPCHK(h, hipMemcpyAsync(o_holder.data() + r0, h->fw_holder, nr * 4, hipMemcpyDeviceToHost, h->s));
            if (next) HIPCHK(h, hipMemcpyAsync(o_next.data() + r0, h->fw_next, nr * 4, hipMemcpyDeviceToHost, h->s));
        }
        HIPCHK(h, evs.mark(h->s));
    }
    HIPCHK(h, hipEventRecord(h->rt_ev[1], h->s));
    HIPCHK(h, stream_sync(h));                                       // the call's one host synchronisation
    HIPCHK(h, hipGetLastError());
    float t = 0;
    HIPCHK(h, hipEventElapsedTime(&t, h->rt_ev[0], h->rt_ev[1]));
    HIPCHK(h, evs.split(&h->fw_split[0], &h->fw_split[1]));
    h->fw_split[2] = 0;
    // key order back to request order: request j * nkeys + k sits at k * nent + j, a listed request i at order[] = i
    auto slot = [&](size_t p) { return key_index ? order[p] : (p % nent) * nkeys + p / nent; };
    for (size_t p = 0; p < nreq; p++) {
        const size_t i = slot(p);
        outcome[i] = o_out[p];
        hops[i] = o_hops[p];
        if (handler) handler[i] = o_handler[p];
        if (holder) holder[i] = o_holder[p];
        if (next) next[i] = o_next[p];
    }
    if (ms) *ms = t;
    return SWIMSIM_OK;
}

int swimsim_forward_census(swimsim_t *h, const uint8_t *keys, const uint64_t *off, size_t nkeys, uint32_t replica_points,
                           uint32_t max_hops, int32_t policy, int32_t mode, uint32_t *counted, uint32_t *outcomes,
                           uint32_t *hops_hist, uint64_t *hist_off, int32_t *hist_handler, uint32_t *hist_count, size_t cap,
                           size_t *nhist, double *ms) {
    if (!h) return SWIMSIM_EINVAL;
    if (!counted || !outcomes || !hops_hist || !hist_off || !nhist || (cap && (!hist_handler || !hist_count)))
        return h->fail(SWIMSIM_EINVAL, "forward census: no output buffer");
    size_t chunk = 0;
    if (int rc = fwd_check(h, keys, off, nkeys, replica_points, max_hops, policy, mode, "forward census", &chunk)) return rc;
    const size_t nbin = nkeys * FWD_NOUT, nhop = nkeys * (max_hops + 1);
    uint32_t all = 0, first = SRC_NONE;
    if (int rc = route_counted(h, SWIMSIM_CENSUS_LIVE, "forward census", nkeys, &all, &first, counted, hist_off, nhist, ms)) return rc;
    const uint32_t ncount = *counted;
    h->fw_split[0] = h->fw_split[1] = h->fw_split[2] = 0;
    if (ncount == 0) {                                               // no entry: every bin is zero
        memset(outcomes, 0, nbin * 4);
        memset(hops_hist, 0, nhop * 4);
        return SWIMSIM_OK;
    }
    DeviceScope ds(h->device);
    // a pass over one key appends at most one pair per row, so a buffer of at least NL pairs always ends the chunking
    const swimsim::RouteTable *tab = nullptr;
    int rc = 0;
    if ((rc = route_exc_scratch(h, h->NL)) || (rc = fwd_table_scratch(h, chunk)) ||
        (rc = route_grow(h, &h->fw_ent, &h->fw_ent_cap, 1, "forward entries")) ||
        (rc = route_grow(h, &h->fw_bins, &h->fw_bins_cap, nbin + nhop, "forward bins")) ||
        (rc = route_keys(h, keys, off, nkeys, replica_points, &tab)))
        return rc;
    uint32_t *d_out = h->fw_bins, *d_hop = h->fw_bins + nbin;
    HIPCHK(h, hipMemcpyAsync(h->fw_ent, &first, 4, hipMemcpyHostToDevice, h->s));
    std::vector<int32_t> base(nkeys);
    FwdEvents evs;
    hipError_t lerr = hipSuccess;
    // a pass: the table of its keys, the base handlers (the chain from the first counted entry), its bins zeroed (a
    // pass that overflows is run again), the chases of every live row
    auto launch = [&](uint32_t k0, uint32_t k1) {
        auto ok = [&](hipError_t e) { if (lerr == hipSuccess) lerr = e; };
        ok(evs.mark(h->s));
        fwd_table(h, tab, nkeys, mode, k0, k1);
        ok(evs.mark(h->s));
        FwdArgs f = fwd_args(h, k0, k1, max_hops, policy);
        f.ent = h->fw_ent;
        f.nent = 1;
        f.nreq = k1 - k0;
        f.handler = h->rt_base + k0;
        hipLaunchKernelGGL(k_fwd_chase<false>, dim3(blocks_for_threads(k1 - k0)), dim3(FWD_THREADS), 0, h->s, h->d, f);
        ok(hipMemcpyAsync(base.data() + k0, h->rt_base + k0, (size_t)(k1 - k0) * 4, hipMemcpyDeviceToHost, h->s));
        ok(hipMemsetAsync(d_out + (size_t)k0 * FWD_NOUT, 0, (size_t)(k1 - k0) * FWD_NOUT * 4, h->s));
        ok(hipMemsetAsync(d_hop + (size_t)k0 * (max_hops + 1), 0, (size_t)(k1 - k0) * (max_hops + 1) * 4, h->s));
        f.handler = nullptr;
        f.base = h->rt_base;
        f.outcomes = d_out;
        f.hops_hist = d_hop;
        route_census_args(h, &f.r, first, all);
        const uint32_t nblk = (h->N + FWD_THREADS - 1) / FWD_THREADS;
        hipLaunchKernelGGL(k_fwd_chase<true>, dim3((k1 - k0) * nblk), dim3(FWD_THREADS), 0, h->s, h->d, f);
        ok(evs.mark(h->s));
    };
    auto one_key_error = [&](unsigned long long cur) {
        return h->fail(SWIMSIM_EHIP, "forward census: %llu exceptions of one key over %u rows", cur, h->NL);
    };
    double total = 0;
    rc = route_census_passes(h, nkeys, launch, route_emit_answers(base, ncount), one_key_error, hist_off, hist_handler, hist_count,
                             cap, nhist, &total, chunk);
    if (rc) return rc;
    HIPCHK(h, lerr);
    HIPCHK(h, hipMemcpyAsync(outcomes, d_out, nbin * 4, hipMemcpyDeviceToHost, h->s));
    HIPCHK(h, hipMemcpyAsync(hops_hist, d_hop, nhop * 4, hipMemcpyDeviceToHost, h->s));
    HIPCHK(h, stream_sync(h));
    HIPCHK(h, evs.split(&h->fw_split[0], &h->fw_split[1]));
    h->fw_split[2] = std::max(0.0, total - h->fw_split[0] - h->fw_split[1]);
    if (ms) *ms = total;
    return SWIMSIM_OK;
}

int swimsim_forward_times(swimsim_t *h, double *table_ms, double *chase_ms, double *hist_ms) {
    if (!h || !table_ms || !chase_ms || !hist_ms) return SWIMSIM_EINVAL;
    *table_ms = h->fw_split[0];
    *chase_ms = h->fw_split[1];
    *hist_ms = h->fw_split[2];
    return SWIMSIM_OK;
}

// ---- ring checksums through the observers' ring views (swimsim_ringcs.hip) ----
namespace {

int ringcs_check(swimsim *h, int32_t mode, const char *what) {
    if (mode < 0 || mode > 2) return h->fail(SWIMSIM_EINVAL, "%s: unknown mode %d", what, mode);
    if (h->N > ROUTE_N_MAX) return h->fail(SWIMSIM_EINVAL, "%s: %u members are more than %u", what, h->N, ROUTE_N_MAX);
    return 0;
}

// the scratch of n requested rows, on first use
int ringcs_scratch(swimsim *h, size_t n) {
    if (n > h->rc_cap) {
        if (h->rc_key) HIPCHK(h, stream_sync(h));
        const size_t o = h->rc_cap;
        auto drop = [&](size_t c) {
            dfree(h, &h->rc_key, dalloc_bytes(c, 8));
            dfree(h, &h->rc_cnt, dalloc_bytes(c, 4));
            dfree(h, &h->rc_rep, dalloc_bytes(c, 4));
            dfree(h, &h->rc_dif, dalloc_bytes(c, 4));
            dfree(h, &h->rc_hl, dalloc_bytes(c, 4));
            dfree(h, &h->rc_csr, dalloc_bytes(c, 4));
            dfree(h, &h->rc_out, dalloc_bytes(c, 4));
        };
        drop(o);
        h->rc_cap = 0;
        const size_t c = n + n / 2;
        int rc = 0;
        if ((rc = dalloc(h, &h->rc_key, c, "ring checksum keys")) || (rc = dalloc(h, &h->rc_cnt, c, "ring checksum server counts")) ||
            (rc = dalloc(h, &h->rc_rep, c, "ring checksum representatives")) || (rc = dalloc(h, &h->rc_dif, c, "ring checksum verify flags")) ||
            (rc = dalloc(h, &h->rc_hl, c, "ring checksum hash list")) || (rc = dalloc(h, &h->rc_csr, c, "ring checksum chains")) ||
            (rc = dalloc(h, &h->rc_out, c, "ring checksums"))) {
            drop(c);                                                 // (a buffer that was not allocated is skipped)
            (void)hipGetLastError();
            return rc;
        }
        h->rc_cap = c;
    }
    if (int rc = route_grow(h, &h->rt_rows, &h->rt_rows_cap, n, "route rows")) return rc;
    for (hipEvent_t &e : h->rt_ev)
        if (!e) HIPCHK(h, hipEventCreate(&e));
    if (!h->rc_lds) {                                                // (N above ~262,000: bitmap and static LDS pass 64 KB)
        if ((size_t)route_bitmap_bytes(h->NP) + RINGCS_STATIC_LDS > 65536) {
            HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_ringcs_hash), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)route_bitmap_bytes(h->NP)));
            HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_ringcs_scan), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)route_bitmap_bytes(h->NP)));
        }
        h->rc_lds = true;
    }
    return 0;
}

// The checksums and server counts of the listed local rows (duplicates allowed), in list order. Three host
// synchronisations at most: the keys, the verify flags (only when some row has a representative other than itself),
// the checksums. *hashed = the chains run.
int ringcs_run(swimsim *h, const std::vector<uint32_t> &rows, int32_t mode, uint32_t *cs, uint32_t *srv, uint32_t *hashed,
               double *ms) {
    const size_t n = rows.size();
    if (int rc = ringcs_scratch(h, n)) return rc;
    const uint32_t nn = (uint32_t)n, lds = route_bitmap_bytes(h->NP);
    float t = 0;
    // 1. scan
    HIPCHK(h, hipMemcpyAsync(h->rt_rows, rows.data(), n * 4, hipMemcpyHostToDevice, h->s));
    HIPCHK(h, hipEventRecord(h->rt_ev[0], h->s));
    hipLaunchKernelGGL(k_ringcs_scan, dim3(nn), dim3(RINGCS_THREADS), lds, h->s, h->d, h->rt_rows, h->rc_key, h->rc_cnt);
    HIPCHK(h, hipEventRecord(h->rt_ev[1], h->s));
    std::vector<unsigned long long> key(n);
    std::vector<uint32_t> cnt(n), rep(n), dif;
    HIPCHK(h, hipMemcpyAsync(key.data(), h->rc_key, n * 8, hipMemcpyDeviceToHost, h->s));
    HIPCHK(h, hipMemcpyAsync(cnt.data(), h->rc_cnt, n * 4, hipMemcpyDeviceToHost, h->s));
    HIPCHK(h, stream_sync(h));                                       // synchronisation 1: 12 bytes per row
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventElapsedTime(&t, h->rt_ev[0], h->rt_ev[1]));
    h->rc_split[0] = t;
    h->rc_split[1] = h->rc_split[2] = 0;
    // 2. group: rows of equal (key, cnt) under their lowest row (mode 2: 3 bits of the key alone; mode 1: no groups)
    bool grouped = false;
    for (uint32_t j = 0; j < nn; j++) rep[j] = j;
    if (mode != 1) {
        std::vector<uint32_t> order(n);
        for (uint32_t j = 0; j < nn; j++) order[j] = j;
        auto gk = [&](uint32_t j) { return mode == 2 ? std::make_pair(key[j] & 7ull, 0u) : std::make_pair(key[j], cnt[j]); };
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
            const auto ka = gk(a), kb = gk(b);
            if (ka != kb) return ka < kb;
            return rows[a] != rows[b] ? rows[a] < rows[b] : a < b;
        });
        for (size_t i = 0; i < n;) {
            size_t e = i + 1;
            while (e < n && gk(order[e]) == gk(order[i])) e++;
            for (size_t q = i; q < e; q++) rep[order[q]] = order[i];
            grouped |= e - i > 1;
            i = e;
        }
    }
    if (grouped) {                                                   // the exact comparison with the representative
        dif.resize(n);
        HIPCHK(h, hipMemcpyAsync(h->rc_rep, rep.data(), n * 4, hipMemcpyHostToDevice, h->s));
        HIPCHK(h, hipMemsetAsync(h->rc_dif, 0, n * 4, h->s));
        HIPCHK(h, hipEventRecord(h->rt_ev[0], h->s));
        hipLaunchKernelGGL(k_ringcs_verify, dim3(nn), dim3(RINGCS_THREADS), 0, h->s, h->d, h->rt_rows, h->rc_rep, nn, h->rc_dif);
        HIPCHK(h, hipEventRecord(h->rt_ev[1], h->s));
        HIPCHK(h, hipMemcpyAsync(dif.data(), h->rc_dif, n * 4, hipMemcpyDeviceToHost, h->s));
        HIPCHK(h, stream_sync(h));                                   // synchronisation 2: 4 bytes per row
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipEventElapsedTime(&t, h->rt_ev[0], h->rt_ev[1]));
        h->rc_split[1] = t;
        for (uint32_t j = 0; j < nn; j++)
            if (dif[j]) rep[j] = j;                                  // a key collision: the row runs its own chain
    }
    // 3. hash the representatives, 4. scatter
    std::vector<uint32_t> hl;
    for (uint32_t j = 0; j < nn; j++)
        if (rep[j] == j) hl.push_back(j);
    HIPCHK(h, hipMemcpyAsync(h->rc_rep, rep.data(), n * 4, hipMemcpyHostToDevice, h->s));
    HIPCHK(h, hipMemcpyAsync(h->rc_hl, hl.data(), hl.size() * 4, hipMemcpyHostToDevice, h->s));
    HIPCHK(h, hipEventRecord(h->rt_ev[0], h->s));
    hipLaunchKernelGGL(k_ringcs_hash, dim3((uint32_t)hl.size()), dim3(RINGCS_THREADS), lds, h->s, h->d, h->rt_rows, h->rc_hl, h->rc_csr);
    hipLaunchKernelGGL(k_ringcs_scatter, dim3(blocks_for_threads(nn)), dim3(256), 0, h->s, h->rc_rep, h->rc_csr, nn, h->rc_out);
    HIPCHK(h, hipEventRecord(h->rt_ev[1], h->s));
    HIPCHK(h, hipMemcpyAsync(cs, h->rc_out, n * 4, hipMemcpyDeviceToHost, h->s));
    HIPCHK(h, stream_sync(h));                                       // synchronisation 3: 4 bytes per row
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventElapsedTime(&t, h->rt_ev[0], h->rt_ev[1]));
    h->rc_split[2] = t;
    if (srv) memcpy(srv, cnt.data(), n * 4);
    if (hashed) *hashed = (uint32_t)hl.size();
    if (ms) *ms = h->rc_split[0] + h->rc_split[1] + h->rc_split[2];
    return SWIMSIM_OK;
}

}  // namespace

int swimsim_ring_checksums(swimsim_t *h, const uint32_t *observers, size_t nobs, int32_t mode, uint32_t *checksums,
                           uint32_t *servers, uint32_t *hashed, double *ms) {
    if (!h) return SWIMSIM_EINVAL;
    if (!checksums) return h->fail(SWIMSIM_EINVAL, "ring checksums: no output buffer");
    if (nobs == 0) return h->fail(SWIMSIM_EINVAL, "ring checksums: no observers");
    if (int rc = ringcs_check(h, mode, "ring checksums")) return rc;
    if (!observers && nobs != h->NL)
        return h->fail(SWIMSIM_EINVAL, "ring checksums: every owned row means nobs = %u, not %zu", h->NL, nobs);
    if (nobs > 0xFFFFFFFFull) return h->fail(SWIMSIM_EINVAL, "ring checksums: list of %zu observers too long", nobs);
    std::vector<uint32_t> rows(nobs);
    for (size_t j = 0; j < nobs; j++) {
        if (observers && (observers[j] < h->lo || observers[j] >= h->lo + h->NL))
            return h->fail(SWIMSIM_EINVAL, "ring checksums: observer %u is not a row of this handle", observers[j]);
        rows[j] = observers ? observers[j] - h->lo : (uint32_t)j;
    }
    DeviceScope ds(h->device);
    std::vector<uint32_t> cs(nobs), srv(nobs);                       // (the outputs are written only by a call that succeeds)
    uint32_t nh = 0;
    double t = 0;
    if (int rc = ringcs_run(h, rows, mode, cs.data(), srv.data(), &nh, &t)) return rc;
    memcpy(checksums, cs.data(), nobs * 4);
    if (servers) memcpy(servers, srv.data(), nobs * 4);
    if (hashed) *hashed = nh;
    if (ms) *ms = t;
    return SWIMSIM_OK;
}

int swimsim_ring_census(swimsim_t *h, int32_t who, int32_t mode, uint32_t *counted, uint32_t *hist_checksum, uint32_t *hist_count,
                        uint32_t *hist_servers, uint32_t *hist_first, size_t cap, size_t *nhist, uint32_t *hashed, double *ms) {
    if (!h) return SWIMSIM_EINVAL;
    if (!counted || !nhist || (cap && (!hist_checksum || !hist_count || !hist_servers || !hist_first)))
        return h->fail(SWIMSIM_EINVAL, "ring census: no output buffer");
    if (who != SWIMSIM_CENSUS_LIVE && who != SWIMSIM_CENSUS_ALL) return h->fail(SWIMSIM_EINVAL, "ring census: unknown who %d", who);
    if (int rc = ringcs_check(h, mode, "ring census")) return rc;
    std::vector<uint32_t> rows;
    for (uint32_t r = 0; r < h->NL; r++)
        if (who == SWIMSIM_CENSUS_ALL || h->live[h->lo + r]) rows.push_back(r);
    const size_t n = rows.size();
    uint32_t nh = 0;
    double t = 0;
    std::vector<uint32_t> cs(n), srv(n);
    if (n) {
        DeviceScope ds(h->device);
        if (int rc = ringcs_run(h, rows, mode, cs.data(), srv.data(), &nh, &t)) return rc;
    }
    // one entry per distinct checksum, ascending; the rows ascend, so the first row of a run is its lowest observer
    std::vector<uint32_t> order(n);
    for (uint32_t j = 0; j < n; j++) order[j] = j;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return cs[a] < cs[b]; });
    size_t total = 0;
    for (size_t i = 0; i < n;) {
        size_t e = i + 1;
        while (e < n && cs[order[e]] == cs[order[i]]) e++;
        if (total < cap) {
            hist_checksum[total] = cs[order[i]];
            hist_count[total] = (uint32_t)(e - i);
            hist_servers[total] = srv[order[i]];
            hist_first[total] = h->lo + rows[order[i]];
        }
        total++;
        i = e;
    }
    *counted = (uint32_t)n;
    *nhist = total;
    if (hashed) *hashed = nh;
    if (ms) *ms = t;
    return SWIMSIM_OK;
}

int swimsim_ring_times(swimsim_t *h, double *scan_ms, double *group_ms, double *hash_ms) {
    if (!h || !scan_ms || !group_ms || !hash_ms) return SWIMSIM_EINVAL;
    *scan_ms = h->rc_split[0];
    *group_ms = h->rc_split[1];
    *hash_ms = h->rc_split[2];
    return SWIMSIM_OK;
}
