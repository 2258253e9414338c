// nt_ctx.hpp -- the per-lane context (Ctx: lane -> (environment, slot), typed LDS accessors, body / shape / dof accessors) and the
// HBM <-> LDS staging helpers of the fused gfx950 kernels.  No include guard: nt_kernels.hip includes this file once per arithmetic
// namespace (after nt_layout.hpp), so that Ctx's own arithmetic (Wsym::quad, update_body_derived) follows the namespace's rules.
// What the block-shared region holds and where is nt_layout.hpp's description (NT_TOPO_TABLE_LIST, topo_region): Ctx binds its pointers to
// it in one step (bind_topology) and fills it from the host-packed image or table by table.
// The tile code EPB of every kernel template carries the environments per workgroup in its low byte and the
// uniform-parameter flag NT_UNI in bit 8: Ctx<EPB>::N is the count, Ctx<EPB>::UNI the flag.
constexpr int NT_UNI = 256;
// Bit 9, NT_SPEC (fused XPBD rollout only): the launch code has verified every fact of xpbd_spec_tile_fits (nt_kernels.hip) for this
// model, these solver options and the granted tile extras, so the kernel takes them as constants instead of testing them in every
// barrier interval: contact records and live list in LDS, pose snapshot granted (integrate_bodies beside the pairs), body phases on
// linear / angular lanes, one pass of uncompacted pairs, no restitution / velocity-from-delta, contacts, joints and iterations present.
// Model sizes, joint types, body flags, iteration count and every float stay run-time values.  Ctx<EPB>::SPEC is the flag.
constexpr int NT_SPEC = 512;
#ifndef NT_ASSUME  // a fact the launch code verified, stated to the optimiser (nothing where the compiler has no such builtin)
#if defined(__clang__)
#define NT_ASSUME(x) __builtin_assume(x)
#else
#define NT_ASSUME(x) ((void)0)
#endif
#endif
// NT_SPEC lane roles: what a lane of that instance is for the whole launch, and the launch-invariant operands of that role, held in
// registers.  A lane's body is fixed there (phase_apply: slot s is angular body s, slot B0 + s linear body s), and what the record
// copies -- the topology region, the block-shared parameter copy -- is written by the prologue alone (bind_topology / load_tile) and by
// no phase.  fused::fill_lane_roles fills it once per launch behind the barriers that publish those regions, from a clamped index (lanes
// without a role read in range and never look at the result), so nothing outlives a launch: parameter edits, new targets and graph
// replays need no invalidation.  Plain values (bit copies of the loaded words); only the XPBD phases' copy of this file uses them.
struct BodyRole {  // the body of an angular lane [0, nb) or a linear lane [B0, B0 + nb) of the apply phases
    int flags;
    int pair_start, pair_count, pair_code0;  // T.body_pair_start[b], the length of the body's list, its first entry (clamped)
    int joint_start, joint_count;            // T.body_joint_start[b], the length of the body's list
    float inv_mass;
    float inv_inertia[9], inertia[9];
};
// ... and of a joint lane: slot j < nj is the linear lane of joint j, slot A0 + j its angular lane (phase_joints), one trip each
// (xpbd_spec_tile_fits: wave_up(nj) + nj <= nslot).  What joint_live finds through four dependent LDS rounds, the two joint frames, the
// dof starts and counts and the joint's two entries of the bodies' incidence lists.
struct JointRole {
    int type, enabled, id_p, id_c;    // T.joint_type / joint_enabled / joint_parent / joint_child [j]
    float inv_mass_p, inv_mass_c;     // (a world-attached parent: 0, as joint_live has it)
    float X_pj[7], X_cj[7];           // L.jp rows 0-6 and 7-13
    int qd_start, tq_start, lin_count, ang_count;
    int ip, ic;                       // T.joint_inc[2 j], [2 j + 1]
};
template <int EPB>
struct Ctx {
    static constexpr int N = EPB & 255;
    static constexpr bool UNI = (EPB & NT_UNI) != 0;
    static constexpr bool SPEC = (EPB & NT_SPEC) != 0;
    static constexpr int SPW = 64 / N > 0 ? 64 / N : 1;  // slots per wave
    const KArgs& a;
    Topo T;
    float* lds;
    float* up;  // UNI: the block-shared parameter copy [L.uni_floats], behind the topology
    LdsLayout L;
    int e, slot, env, nslot;
    int tslot;  // start of the item loop of phases with fewer items than slot-threads.  Identity: dealing consecutive items to
                // DIFFERENT waves (13 bodies x 16 envs on all 8 waves instead of 4) was measured and lost 13 % on the headline
                // (87.4 vs 100.8 M env-steps/s) -- twice the wave-instructions cost more than the second wave per SIMD hides
    int pose_in_off;  // rows of the poses the contact writer converts into (collide.py:166-204: the step's incoming poses): L.bq, or the
                      // snapshot L.xiq while integrate_bodies runs beside the pair phase of a fused rollout
    bool lane_split;    // the XPBD body phases may run on linear / angular lanes (false in the convex kernels: they sit at the register
                        // limit, and the second copy of the body phases costs them more in spills than the idle waves give back)
    bool gworld_ready;  // T.gworld holds the global shapes' world transforms / AABBs (stage_global_world ran, a barrier ago)
    bool lds_records;  // NT_TILE_LDS_RECORDS granted: the contact records of this launch live in L.cr
    bool hbm_out;      // the collide phases write the Contacts buffers in HBM (always, except the non-final substeps of an LDS-record rollout)
    bool aos_records;  // pair-heavy fused rollout: the substep's contact records live in nt_contacts.cr (one line per slot); hbm_out then
                       // only holds for the last substep
    bool big;  // contact records in HBM, manifold polygon scratch per lane (compile-time constant at every construction site)
    // The flags above that xpbd_spec_tile_fits fixes, as the phases ask for them: constants on the NT_SPEC instance (records and live
    // list in LDS, a staged tile), the members everywhere else.  hbm_out changes inside a launch and stays a plain member.
    NT_DI bool has_lds_records() const { if constexpr (SPEC) return true; else return lds_records; }
    NT_DI bool has_aos_records() const { if constexpr (SPEC) return false; else return aos_records; }
    NT_DI bool is_big() const { if constexpr (SPEC) return false; else return big; }
    NT_DI bool has_live_list() const { if constexpr (SPEC) return true; else return L.has_lt != 0; }
    int ES;
    bool valid;
    // launch-invariant slot ranges (first slot of the second population of a shared interval, on a wave boundary), computed once here
    // instead of in every barrier interval.  Read by the NT_SPEC instance only; everywhere else the phases derive them in place
    struct Ranges { int B0, S0, I0, A0; } R;  // linear body lanes, joint-force lanes, integrate lanes, angular joint lanes
    // the lane's role (NT_SPEC only: fused::fill_lane_roles on the XPBD phases' context; never set, copied or read anywhere else)
    BodyRole rb;
    JointRole rj;

    // rows: float rows per env in front of the block-shared topology ints (-1: the XPBD / collide layout)
    // defer_image: the kernel calls load_tile next (see issue_image)
    NT_DI Ctx(const KArgs& a_, float* lds_, int rows = -1, const bool big_ = false, const bool defer_image = false) : a(a_), lds(lds_), big(big_) {
        // (rows >= 0: another solver's layout, no live list; the pair-heavy tile sizes its per-lane polygon scratch by the workgroup
        // the launch code chose: 256 lanes, or NT_BIG_SCENE_LANES_WIDE when they fit)
        L = make_layout(a.m, big_, xpbd_keeps_prestep_state(a.p), UNI, rows < 0, a.tile_opts,
                        big_ && (int)blockDim.x > NT_BIG_SCENE_LANES ? NT_BIG_SCENE_LANES_WIDE : NT_BIG_SCENE_LANES);
        pose_in_off = L.bq.off;
        lds_records = rows < 0 && (a.tile_opts & NT_TILE_LDS_RECORDS) != 0;
        hbm_out = true;
        aos_records = false;
        if (rows < 0) rows = L.rows_per_env;
        e = threadIdx.x % N;
        slot = threadIdx.x / N;
        nslot = a.nslot;
        env = blockIdx.x * N + e;
        ES = a.m.env_stride;
        valid = env < a.m.env_count && slot < nslot;
        tslot = slot;
        const nt_model& m = a.m;
        R = {wave_up(m.nb), wave_up(m.ns), wave_up(m.np), wave_up(m.nj)};
        ti = reinterpret_cast<int*>(lds + (size_t)rows * N);
        gworld_ready = false;
        lane_split = true;
        has_image = IMAGE && m.tile_image_words >= topo_words();  // (the image then starts at m.body_flags)
        img.pending = img.params = false;
        // (bind_topology runs once on either path: in front of the image's loads, or inside stage_topology behind its batch of 24
        // loaded values, which is the register peak of several kernels -- profiles/topo_region_resources.txt)
        if (IMAGE && has_image) {
            bind_topology();
            issue_image(defer_image);
        } else {
            stage_topology();
        }
    }
    // The tiles of 32 and 64 environments keep the table-by-table staging: with the image code in them the substep loop of the
    // 32-wide rollout instance was scheduled 4 % slower (8 192 / 65 536 quadrupeds: 249.1 -> 239.5 M env-steps/s with NT_TILE_IMAGE=0,
    // 246.7 with the image; profiles/tile_image_ab.txt), more than the shorter prologue gives back at two workgroups per CU and more.
    static constexpr bool IMAGE = N < 32;
    // nt_model.tile_image_words set (the image starts at m.body_flags): the block-shared region is one copy.  Every lane issues its 16-byte loads of the image
    // (workgroup-strided, the first NT_IMAGE_TRIPS of them in flight together) before the first LDS write; T.* and `up` are plain
    // offsets.  The gworld range and the pair-heavy tile's hit list stay unwritten (stage_global_world / the pair-heavy kernels fill
    // them).  defer: the kernel calls load_tile next and leaves `up` where it is (the collide / XPBD kernels) -- the stores wait for
    // commit_image(), which load_tile calls behind ITS loads, so that image, state and controls are one memory round trip, and the
    // image's parameter block is taken.  Kernels of the other solvers put tables of their own behind the topology and move `up`
    // behind those: they take the topology part only and load the parameter copy as without an image.
    // 4-byte LDS stores: the region starts behind rows * N floats, 16-byte aligned for some N only.
    static constexpr int NT_IMAGE_TRIPS = 2;
    struct Image {
        TileImageQuad v[NT_IMAGE_TRIPS];
        int total;           // words to copy: the topology [+ the parameter block of a uniform-parameter tile]
        int g0, g1, h0, h1;  // the two ranges left unwritten
        bool pending;        // loads issued, stores outstanding
        bool params;         // the image fills `up`: load_uniform_params has nothing to do
    };
    mutable Image img;
    int* ti;
    bool has_image;
    // where the parts of the block-shared region live (topo_region, nt_layout.hpp), whichever way they are filled: T.*, `up` behind
    // them, and the two ranges an image copy leaves unwritten (gworld; the pair-heavy tile's hit list)
    NT_DI void bind_topology() {
        const nt_model& m = a.m;
        const TopoRegion tr = topo_region(m);
        topo_bind_tables(T, m, ti);
        T.gshape = reinterpret_cast<float*>(ti + tr.gshape);
        T.gworld = reinterpret_cast<float*>(ti + tr.gworld);
        T.joint_inc = ti + tr.joint_inc;
        T.hit_count = ti + tr.tail;
        T.hit_list = ti + tr.tail + 1;
        T.pair_desc = ti + tr.tail;  // (the two tables exclude each other)
        up = reinterpret_cast<float*>(ti + topo_words());
        img.g0 = tr.gworld;
        img.g1 = tr.joint_inc;
        img.h0 = m.contact_scratch_in_hbm ? tr.tail : tr.total;
        img.h1 = tr.total;
    }
    // words of the region.  The tiles that never take the image use the closed form: with `up` derived from the walked sum the
    // substep loop of the 32-wide XPBD rollout reloads more spilled scalars, -4.5 % at 8 192 environments; the image tiles keep the
    // walked total, with which the tile of 16 measures as before (profiles/topo_region_ab.txt)
    NT_DI int topo_words() const { return IMAGE ? topo_region(a.m).total : topo_ints(a.m); }
    // a kernel's own block-shared tables: n ints just behind the topology; the uniform parameter copy moves behind them
    NT_DI int* own_tables(const int n) {
        int* const tab = ti + topo_words();
        up = reinterpret_cast<float*>(tab + n);
        return tab;
    }
    NT_DI void issue_image(const bool defer) {
        const nt_model& m = a.m;
        img.total = img.h1;
        if constexpr (UNI) {
            if (defer && m.tile_image_words >= img.total + L.uni_floats) {
                img.total += L.uni_floats;
                img.params = true;
            }
        }
        const TileImageQuad* src = reinterpret_cast<const TileImageQuad*>(m.body_flags);
        const int n4 = (img.total + 3) / 4;  // (the image is readable up to a multiple of four words)
#pragma unroll
        for (int k = 0; k < NT_IMAGE_TRIPS; ++k) {
            const int i4 = (int)threadIdx.x + k * (int)blockDim.x;
            img.v[k] = i4 < n4 ? src[i4] : TileImageQuad{{0, 0, 0, 0}};
        }
        img.pending = true;
        if (!defer) commit_image();
    }
    NT_DI void image_store(const int i4, const TileImageQuad& v) const {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int w = 4 * i4 + k;
            if (w < img.total && !(w >= img.g0 && w < img.g1) && !(w >= img.h0 && w < img.h1)) ti[w] = v.w[k];
        }
    }
    NT_DI void commit_image() const {
        if (!img.pending) return;
        img.pending = false;
        const int n4 = (img.total + 3) / 4;
#pragma unroll
        for (int k = 0; k < NT_IMAGE_TRIPS; ++k) {
            const int i4 = (int)threadIdx.x + k * (int)blockDim.x;
            if (i4 < n4) image_store(i4, img.v[k]);
        }
        const TileImageQuad* src = reinterpret_cast<const TileImageQuad*>(a.m.body_flags);
        for (int i4 = (int)threadIdx.x + NT_IMAGE_TRIPS * (int)blockDim.x; i4 < n4; i4 += blockDim.x) image_store(i4, src[i4]);
    }
    // no image (nt_model.tile_image_words == 0): the region is staged table by table from the descriptor's own tables
    NT_DI void stage_topology() {
        const nt_model& m = a.m;
        int o = 0;
        // The 24 env-uniform tables are fetched FIRST -- every thread one element of each, all loads in flight together -- and
        // written to LDS afterwards.  (One copy loop per table compiles to load / s_waitcnt vmcnt(0) / ds_write per table: 24
        // serialised memory round trips, ~25 us per launch -- most of what a per-call collide / step kernel took, 8 % of a
        // 10-substep rollout launch.)  Tables longer than the workgroup finish in a tail loop.
        const TopoTables tt = topo_tables(m);
        int first[NT_TOPO_TABLES];
        const int tid = threadIdx.x;
#pragma unroll
        for (int k = 0; k < NT_TOPO_TABLES; ++k) first[k] = tid < tt.len[k] ? tt.src[k][tid] : 0;
        const int ngf = NT_SHAPE_PARAM_FLOATS * m.ng;
        const float gfirst = tid < ngf ? m.gshape_param[tid] : 0.0f;
#pragma unroll
        for (int k = 0; k < NT_TOPO_TABLES; ++k) {
            if (tid < tt.len[k]) ti[o + tid] = first[k];
            for (int i = tid + (int)blockDim.x; i < tt.len[k]; i += blockDim.x) ti[o + i] = tt.src[k][i];
            o += tt.len[k];
        }
        float* g = reinterpret_cast<float*>(ti + o);  // (behind the tables: what bind_topology makes T.gshape)
        if (tid < ngf) g[tid] = gfirst;
        for (int i = tid + (int)blockDim.x; i < ngf; i += blockDim.x) g[i] = m.gshape_param[i];
        bind_topology();
        // (joint_inc is filled by stage_joint_inc, one barrier after the tables above are published)
        if (!m.contact_scratch_in_hbm)
            for (int i = threadIdx.x; i < m.np; i += blockDim.x) pair_desc_words(m, i, const_cast<int*>(T.pair_desc) + 4 * i);
    }
    // the same lane seen from the other arithmetic namespace (ieee::Ctx <-> fused::Ctx): no staging, every member copied
    template <class OtherCtx>
    NT_DI explicit Ctx(const OtherCtx& o, int /*tag*/)
        : a(o.a), T(o.T), lds(o.lds), up(o.up), L(o.L), e(o.e), slot(o.slot), env(o.env), nslot(o.nslot), tslot(o.tslot),
          pose_in_off(o.pose_in_off), lane_split(o.lane_split), gworld_ready(o.gworld_ready), lds_records(o.lds_records), hbm_out(o.hbm_out), aos_records(o.aos_records), big(o.big),
          ES(o.ES), valid(o.valid), R{o.R.B0, o.R.S0, o.R.I0, o.R.A0}, ti(o.ti), has_image(o.has_image) {
        img.pending = false;  // (the staging belongs to the lane's first context)
        img.params = o.img.params;
    }
    static NT_DI int wave_up(int n) { return ((n + SPW - 1) / SPW) * SPW; }  // n rounded up to whole waves of slots
    // LDS element (comp, s) of a slot-major field.  `n` (the slot count of the [comp][n] HBM twin) is not needed here; the
    // argument stays so that every access reads like its global-memory counterpart g(comp, n, s)
    template <int NC>
    NT_DI float& l(Fld<NC> f, int comp, int /*n*/, int s) const { return lds[(f.off + s * NC + comp) * N + e]; }
    // parameter element (fields bp / jp / dp / sp): per-environment row, or the block-shared copy of a uniform tile
    template <int NC>
    NT_DI float pl(Fld<NC> f, int comp, int /*n*/, int s) const {
        if constexpr (UNI) return up[f.off + s * NC + comp];
        else return lds[(f.off + s * NC + comp) * N + e];
    }
    template <int NC>
    NT_DI vec3 plv3(Fld<NC> f, int comp0, int n, int s) const {
        return vec3(pl(f, comp0, n, s), pl(f, comp0 + 1, n, s), pl(f, comp0 + 2, n, s));
    }
    template <int NC>
    NT_DI xform plxf(Fld<NC> f, int comp0, int n, int s) const {
        return xform(plv3(f, comp0, n, s),
                     quat(pl(f, comp0 + 3, n, s), pl(f, comp0 + 4, n, s), pl(f, comp0 + 5, n, s), pl(f, comp0 + 6, n, s)));
    }
    template <int NC>
    NT_DI mat33 plm33(Fld<NC> f, int comp0, int n, int s) const {
        return mat33(pl(f, comp0, n, s), pl(f, comp0 + 1, n, s), pl(f, comp0 + 2, n, s), pl(f, comp0 + 3, n, s),
                     pl(f, comp0 + 4, n, s), pl(f, comp0 + 5, n, s), pl(f, comp0 + 6, n, s), pl(f, comp0 + 7, n, s),
                     pl(f, comp0 + 8, n, s));
    }
    NT_DI size_t g(int comp, int n, int s) const { return (size_t)(comp * n + s) * ES + env; }

    template <int NC>
    NT_DI vec3 lv3(Fld<NC> f, int comp0, int n, int s) const {
        return vec3(l(f, comp0, n, s), l(f, comp0 + 1, n, s), l(f, comp0 + 2, n, s));
    }
    template <int NC>
    NT_DI void st_lv3(Fld<NC> f, int comp0, int n, int s, vec3 v) const {
        l(f, comp0, n, s) = v.x; l(f, comp0 + 1, n, s) = v.y; l(f, comp0 + 2, n, s) = v.z;
    }
    template <int NC>
    NT_DI xform lxf(Fld<NC> f, int comp0, int n, int s) const {
        return xform(lv3(f, comp0, n, s),
                     quat(l(f, comp0 + 3, n, s), l(f, comp0 + 4, n, s), l(f, comp0 + 5, n, s), l(f, comp0 + 6, n, s)));
    }
    template <int NC>
    NT_DI void st_lxf(Fld<NC> f, int n, int s, const xform& t) const {
        l(f, 0, n, s) = t.p.x; l(f, 1, n, s) = t.p.y; l(f, 2, n, s) = t.p.z;
        l(f, 3, n, s) = t.q.x; l(f, 4, n, s) = t.q.y; l(f, 5, n, s) = t.q.z; l(f, 6, n, s) = t.q.w;
    }
    template <int NC>
    NT_DI mat33 lm33(Fld<NC> f, int comp0, int n, int s) const {
        return mat33(l(f, comp0, n, s), l(f, comp0 + 1, n, s), l(f, comp0 + 2, n, s), l(f, comp0 + 3, n, s),
                     l(f, comp0 + 4, n, s), l(f, comp0 + 5, n, s), l(f, comp0 + 6, n, s), l(f, comp0 + 7, n, s),
                     l(f, comp0 + 8, n, s));
    }
    NT_DI vec3 gravity() const { return lv3(L.grav, 0, 1, 0); }
    // component-major [comp][n] arrays at a plain row offset (a solver's own scratch, e.g. SolverFeatherstone's)
    NT_DI float& l(int off, int comp, int n, int s) const { return lds[(off + comp * n + s) * N + e]; }
    NT_DI vec3 lv3(int off, int comp0, int n, int s) const {
        return vec3(l(off, comp0, n, s), l(off, comp0 + 1, n, s), l(off, comp0 + 2, n, s));
    }
    NT_DI void st_lv3(int off, int comp0, int n, int s, vec3 v) const {
        l(off, comp0, n, s) = v.x; l(off, comp0 + 1, n, s) = v.y; l(off, comp0 + 2, n, s) = v.z;
    }
    NT_DI xform lxf(int off, int comp0, int n, int s) const {
        return xform(lv3(off, comp0, n, s),
                     quat(l(off, comp0 + 3, n, s), l(off, comp0 + 4, n, s), l(off, comp0 + 5, n, s), l(off, comp0 + 6, n, s)));
    }
    NT_DI void st_lxf(int off, int n, int s, const xform& t) const {
        l(off, 0, n, s) = t.p.x; l(off, 1, n, s) = t.p.y; l(off, 2, n, s) = t.p.z;
        l(off, 3, n, s) = t.q.x; l(off, 4, n, s) = t.q.y; l(off, 5, n, s) = t.q.z; l(off, 6, n, s) = t.q.w;
    }
    NT_DI vec3 gv3(const float* base, int comp0, int n, int s) const {
        return vec3(base[g(comp0, n, s)], base[g(comp0 + 1, n, s)], base[g(comp0 + 2, n, s)]);
    }

    // inverse of body_joint_list: position of code (j << 1 | side) in the list, -1 for the world side of a root joint.  Reads the
    // block-shared copy of the list, i.e. runs one barrier after the constructor; the XPBD joint phases are barriers later still
    NT_DI void stage_joint_inc() const {
        if (has_image) return;  // (the image carries the table)
        const int nlist = a.m.nj > 0 ? T.body_joint_start[a.m.nb] : 0;
        int* inv = const_cast<int*>(T.joint_inc);
        for (int i = threadIdx.x; i < 2 * a.m.nj; i += blockDim.x) inv[i] = joint_inc_entry(T.body_joint_list, nlist, i);
    }
    NT_DI xform body_q(int b) const { return lxf(L.bq, 0, a.m.nb, b); }
    // the step's incoming pose of body b.  NT_SPEC: the rotation from the snapshot rows, the origin from L.bq -- an apply phase follows
    // (verified by the launch code), so inside a step the origins (rows 0..2) are written by the step's last apply alone, and the
    // snapshot holds rows 3..6 only (xpbd_integrate_item<EPB, true> fills them)
    NT_DI xform body_q_in(int b) const {
        if constexpr (SPEC) {
            const int nb = a.m.nb;
            const Fld<7> in{pose_in_off};  // (L.xiq on this instance)
            return xform(lv3(L.bq, 0, nb, b), quat(l(in, 3, nb, b), l(in, 4, nb, b), l(in, 5, nb, b), l(in, 6, nb, b)));
        } else {
            return lxf(Fld<7>{pose_in_off}, 0, a.m.nb, b);
        }
    }
    NT_DI quat body_rot(int b) const {
        const int nb = a.m.nb;
        return quat(l(L.bq, 3, nb, b), l(L.bq, 4, nb, b), l(L.bq, 5, nb, b), l(L.bq, 6, nb, b));
    }
    NT_DI vec3 body_v(int b) const { return lv3(L.bqd, 0, a.m.nb, b); }
    NT_DI vec3 body_w(int b) const { return lv3(L.bqd, 3, a.m.nb, b); }
    NT_DI float inv_mass(int b) const { return pl(L.bp, BP_INV_MASS, a.m.nb, b); }
    NT_DI mat33 inv_inertia(int b) const { return plm33(L.bp, BP_INV_INERTIA, a.m.nb, b); }
    NT_DI mat33 inertia(int b) const { return plm33(L.bp, BP_INERTIA, a.m.nb, b); }
    NT_DI vec3 com(int b) const { return plv3(L.bp, BP_COM, a.m.nb, b); }
    NT_DI vec3 world_com(int b) const { return lv3(L.bd, 0, a.m.nb, b); }
    // the world-frame inverse inertia tile R I^-1 R^T of body b as a value (six floats fetched once, then any number of quadratic
    // forms v^T W v)
    struct Wsym {
        float xx, xy, xz, yy, yz, zz;
        NT_DI float quad(vec3 v) const {
            vec3 wv(xx * v.x + xy * v.y + xz * v.z, xy * v.x + yy * v.y + yz * v.z, xz * v.x + yz * v.y + zz * v.z);
            return dot(v, wv);
        }
    };
    NT_DI Wsym w_tile(int b) const {
        const int nb = a.m.nb;
        return Wsym{l(L.bd, 3, nb, b), l(L.bd, 4, nb, b), l(L.bd, 5, nb, b), l(L.bd, 6, nb, b), l(L.bd, 7, nb, b), l(L.bd, 8, nb, b)};
    }
    NT_DI void update_body_derived(int b) const {
        xform X = body_q(b);
        update_world_com(b, X);
        update_body_w(b, X.q);
    }
    // world COM of body b at pose X (the first three rows of the body-derived tile)
    NT_DI void update_world_com(int b, const xform& X) const { st_lv3(L.bd, 0, a.m.nb, b, xform_point(X, com(b))); }
    // W = R I^-1 R^T of body b at rotation q (rows 3..8 of the tile)
    NT_DI void update_body_w(int b, quat q) const {
        const int nb = a.m.nb;
        mat33 R = quat_to_matrix(q);
        mat33 Ii = inv_inertia(b);
        // T = I^-1 R^T ; W = R T
        vec3 t0 = Ii * vec3(R.m00, R.m01, R.m02), t1 = Ii * vec3(R.m10, R.m11, R.m12), t2 = Ii * vec3(R.m20, R.m21, R.m22);
        vec3 r0(R.m00, R.m01, R.m02), r1(R.m10, R.m11, R.m12), r2(R.m20, R.m21, R.m22);
        l(L.bd, 3, nb, b) = dot(r0, t0); l(L.bd, 4, nb, b) = dot(r0, t1); l(L.bd, 5, nb, b) = dot(r0, t2);
        l(L.bd, 6, nb, b) = dot(r1, t1); l(L.bd, 7, nb, b) = dot(r1, t2); l(L.bd, 8, nb, b) = dot(r2, t2);
    }
    // the same with the body-frame inverse inertia in the caller's registers (NT_SPEC lane roles: BodyRole::inv_inertia)
    NT_DI void update_body_w(int b, quat q, const mat33& Ii) const {
        const int nb = a.m.nb;
        mat33 R = quat_to_matrix(q);
        vec3 t0 = Ii * vec3(R.m00, R.m01, R.m02), t1 = Ii * vec3(R.m10, R.m11, R.m12), t2 = Ii * vec3(R.m20, R.m21, R.m22);
        vec3 r0(R.m00, R.m01, R.m02), r1(R.m10, R.m11, R.m12), r2(R.m20, R.m21, R.m22);
        l(L.bd, 3, nb, b) = dot(r0, t0); l(L.bd, 4, nb, b) = dot(r0, t1); l(L.bd, 5, nb, b) = dot(r0, t2);
        l(L.bd, 6, nb, b) = dot(r1, t1); l(L.bd, 7, nb, b) = dot(r1, t2); l(L.bd, 8, nb, b) = dot(r2, t2);
    }
    NT_DI float dof(int row, int d) const { return pl(L.dp, row, a.m.nd, d); }
    NT_DI vec3 dof_axis(int d) const { return plv3(L.dp, DP_AXIS, a.m.nd, d); }

    // shape accessors: s < ns local (per-env params in LDS), otherwise the env-uniform global table
    NT_DI float shape_f(int s, int comp) const {
        if (s < a.m.ns) return pl(L.sp, comp, a.m.ns, s);
        return T.gshape[(s - a.m.ns) * NT_SHAPE_PARAM_FLOATS + comp];
    }
    // the same value through ONE load from a selected LDS address (no branch between the two tables: the loads of a phase's operands
    // then leave as one batch)
    NT_DI float shape_f_sel(int s, int comp) const {
        const float* local;
        if constexpr (UNI) local = up + (L.sp.off + s * NC_SP + comp);
        else local = lds + ((L.sp.off + s * NC_SP + comp) * N + e);
        const float* global = T.gshape + ((s - a.m.ns) * NT_SHAPE_PARAM_FLOATS + comp);
        return *(s < a.m.ns ? local : global);
    }
    NT_DI vec3 shape_scale(int s) const { return vec3(shape_f(s, SP_SCALE), shape_f(s, SP_SCALE + 1), shape_f(s, SP_SCALE + 2)); }
    NT_DI xform shape_local_xform(int s) const {
        return xform(vec3(shape_f(s, 0), shape_f(s, 1), shape_f(s, 2)), quat(shape_f(s, 3), shape_f(s, 4), shape_f(s, 5), shape_f(s, 6)));
    }
    NT_DI int newton_shape_id(int s) const {  // flat Newton shape index
        return s < a.m.ns ? a.m.shape_local0 + env * a.m.ns + s : T.gshape_id[s - a.m.ns];
    }
    NT_DI int local_shape_id(int gid) const {
        int rel = gid - a.m.shape_local0 - env * a.m.ns;
        if (rel >= 0 && rel < a.m.ns) return rel;
        int g = 0;
        for (int k = 0; k < a.m.ng; ++k)
            if (T.gshape_id[k] == gid) g = k;
        return a.m.ns + g;
    }
};

// ------------------------------------------------------------------------------------------------
// HBM <-> LDS staging
// ------------------------------------------------------------------------------------------------
// field [ncomp][n][ES] in HBM <-> slot-major rows in LDS
// (loads in batches of eight before the LDS writes: a load / wait / write per row is one memory round trip per row)
// first: the first item of the lane's walk -- c.slot, or c.slot + c.nslot behind a first trip that load_tile fetched itself
constexpr int NT_STAGE_BATCH = 8;
template <int EPB, int NC>
NT_DI void stage_rows(const Ctx<EPB>& c, Fld<NC> f, const float* src, int ncomp, int n, int first) {
    for (int s = first; s < n; s += c.nslot)
        for (int c0 = 0; c0 < ncomp; c0 += NT_STAGE_BATCH) {
            float v[NT_STAGE_BATCH];
#pragma unroll
            for (int k = 0; k < NT_STAGE_BATCH; ++k) v[k] = c0 + k < ncomp ? src[c.g(c0 + k, n, s)] : 0.0f;
#pragma unroll
            for (int k = 0; k < NT_STAGE_BATCH; ++k)
                if (c0 + k < ncomp) c.l(f, c0 + k, n, s) = v[k];
        }
}
template <int EPB, int NC>
NT_DI void unstage_rows(const Ctx<EPB>& c, Fld<NC> f, float* dst, int ncomp, int n) {
    for (int comp = 0; comp < ncomp; ++comp)
        for (int s = c.slot; s < n; s += c.nslot) dst[c.g(comp, n, s)] = c.l(f, comp, n, s);
}
// plain rows (a solver's own [row] arrays)
template <int EPB>
NT_DI void stage_rows(const Ctx<EPB>& c, int lds_off, const float* src, int rows) {
    for (int r0 = c.slot; r0 < rows; r0 += NT_STAGE_BATCH * c.nslot) {
        float v[NT_STAGE_BATCH];
#pragma unroll
        for (int k = 0; k < NT_STAGE_BATCH; ++k) v[k] = r0 + k * c.nslot < rows ? src[(size_t)(r0 + k * c.nslot) * c.ES + c.env] : 0.0f;
#pragma unroll
        for (int k = 0; k < NT_STAGE_BATCH; ++k)
            if (r0 + k * c.nslot < rows) c.lds[(lds_off + r0 + k * c.nslot) * Ctx<EPB>::N + c.e] = v[k];
    }
}
template <int EPB>
NT_DI void unstage_rows(const Ctx<EPB>& c, int lds_off, float* dst, int rows) {
    for (int r = c.slot; r < rows; r += c.nslot) dst[(size_t)r * c.ES + c.env] = c.lds[(lds_off + r) * Ctx<EPB>::N + c.e];
}
// the body parameters of the lane's environment from item `first` on, inverse mass / inertia as effective_body_param gives them
// (flags from the descriptor's table: the LDS topology may not be published yet); BATCH components' loads leave together
template <int BATCH, int EPB>
NT_DI void stage_body_params(const Ctx<EPB>& c, int first) {
    const nt_model& m = c.a.m;
    for (int b = first; b < m.nb; b += c.nslot)
        for (int c0 = 0; c0 < NT_BODY_PARAM_FLOATS; c0 += BATCH) {
            float v[BATCH];
#pragma unroll
            for (int k = 0; k < BATCH; ++k)
                v[k] = c0 + k < NT_BODY_PARAM_FLOATS ? effective_body_param(c0 + k, m.body_flags[b], m.body_param[c.g(c0 + k, m.nb, b)]) : 0.0f;
#pragma unroll
            for (int k = 0; k < BATCH; ++k)
                if (c0 + k < NT_BODY_PARAM_FLOATS) c.l(c.L.bp, c0 + k, m.nb, b) = v[k];
        }
}

template <int EPB>
NT_DI void load_state(const Ctx<EPB>& c, const nt_state& s) {
    if (!c.valid) return;
    stage_rows(c, c.L.bq, s.body_q, 7, c.a.m.nb, c.slot);
    stage_rows(c, c.L.bqd, s.body_qd, 6, c.a.m.nb, c.slot);
}
template <int EPB>
NT_DI void store_state(const Ctx<EPB>& c, const nt_state& s) {
    if (!c.valid) return;
    unstage_rows(c, c.L.bq, s.body_q, 7, c.a.m.nb);
    unstage_rows(c, c.L.bqd, s.body_qd, 6, c.a.m.nb);
}
// ---- first-trip batches: the first item a lane owns in a field (s = slot), all components at once.  A kernel's whole tile -- state,
// parameters, controls -- is fetched as ONE batch of loads followed by the LDS writes (load_tile); items beyond the first trip
// (fields longer than the slot-thread count) follow through stage_rows / stage_body_params from c.slot + c.nslot.
template <int NCOMP, int EPB>
NT_DI void first_load(const Ctx<EPB>& c, const float* src, int n, float (&v)[NCOMP]) {
#pragma unroll
    for (int k = 0; k < NCOMP; ++k) v[k] = c.slot < n ? src[c.g(k, n, c.slot)] : 0.0f;
}
template <int NCOMP, int EPB, int NC>
NT_DI void first_store(const Ctx<EPB>& c, Fld<NC> f, int n, const float (&v)[NCOMP]) {
    if (c.slot < n) {
#pragma unroll
        for (int k = 0; k < NCOMP; ++k) c.l(f, k, n, c.slot) = v[k];
    }
}

// the block-shared parameter copy of a uniform-parameter tile: one copy per workgroup, read from the tile's first environment (the
// host vouches that all columns are equal), laid out by uni_word.  Only where the tile image does not hold the copy
template <int EPB>
NT_DI void load_uniform_params(const Ctx<EPB>& c) {
    if (c.img.params) return;  // (the tile image carried the copy: nt_model.tile_image_words)
    const nt_model& m = c.a.m;
    const size_t col = (size_t)blockIdx.x * Ctx<EPB>::N;
    auto at = [&](const float* table, int r) { return table[(size_t)r * c.ES + col]; };
    // (flags from the descriptor's table: the LDS topology is not published yet)
    auto body = [&](int r) { return effective_body_param(r / m.nb, m.body_flags[r % m.nb], at(m.body_param, r)); };
    const int nbp = NT_BODY_PARAM_FLOATS * m.nb, njp = NT_JOINT_PARAM_FLOATS * m.nj, ndp = NT_DOF_PARAM_FLOATS * m.nd,
              nsp = NT_SHAPE_PARAM_FLOATS * m.ns;
    const int r0 = threadIdx.x, step = blockDim.x;
    // first trip of the four tables as one batch of loads, then the rest
    const float vb = r0 < nbp ? body(r0) : 0.0f;
    const float vj = r0 < njp ? at(m.joint_param, r0) : 0.0f;
    const float vd = r0 < ndp ? at(m.dof_param, r0) : 0.0f;
    const float vs = r0 < nsp ? at(m.shape_param, r0) : 0.0f;
    if (r0 < nbp) c.up[uni_word(c.L.bp, r0, m.nb)] = vb;
    if (r0 < njp) c.up[uni_word(c.L.jp, r0, m.nj)] = vj;
    if (r0 < ndp) c.up[uni_word(c.L.dp, r0, m.nd)] = vd;
    if (r0 < nsp) c.up[uni_word(c.L.sp, r0, m.ns)] = vs;
    for (int r = r0 + step; r < nbp; r += step) c.up[uni_word(c.L.bp, r, m.nb)] = body(r);
    for (int r = r0 + step; r < njp; r += step) c.up[uni_word(c.L.jp, r, m.nj)] = at(m.joint_param, r);
    for (int r = r0 + step; r < ndp; r += step) c.up[uni_word(c.L.dp, r, m.nd)] = at(m.dof_param, r);
    for (int r = r0 + step; r < nsp; r += step) c.up[uni_word(c.L.sp, r, m.ns)] = at(m.shape_param, r);
}
// parameters and controls: read once per kernel
template <int EPB>
NT_DI void load_params(const Ctx<EPB>& c, bool with_control) {
    const nt_model& m = c.a.m;
    if constexpr (Ctx<EPB>::UNI) load_uniform_params(c);
    if (!c.valid) return;
    if constexpr (!Ctx<EPB>::UNI) {
        stage_body_params<NT_STAGE_BATCH>(c, c.slot);
        stage_rows(c, c.L.jp, m.joint_param, NT_JOINT_PARAM_FLOATS, m.nj, c.slot);
        stage_rows(c, c.L.dp, m.dof_param, NT_DOF_PARAM_FLOATS, m.nd, c.slot);
        stage_rows(c, c.L.sp, m.shape_param, NT_SHAPE_PARAM_FLOATS, m.ns, c.slot);
    }
    stage_rows(c, c.L.grav, m.gravity, 3, 1, c.slot);
    if (with_control) {
        stage_rows(c, c.L.cf, c.a.c.joint_f, 1, m.nd, c.slot);
        stage_rows(c, c.L.ctq, c.a.c.joint_target_q, 1, m.ntq, c.slot);
        stage_rows(c, c.L.ctqd, c.a.c.joint_target_qd, 1, m.nd, c.slot);
    }
}

// state (optional) + parameters + gravity + controls of the lane's environment in one batch of loads (see first_load): what the XPBD /
// collide kernels call instead of load_state + load_params
template <int EPB>
NT_DI void load_tile(const Ctx<EPB>& c, const nt_state* state, bool with_control) {
    const nt_model& m = c.a.m;
    const int nb = m.nb;
    constexpr bool UNI = Ctx<EPB>::UNI;
    if constexpr (UNI) load_uniform_params(c);  // (the block-shared parameter copy: workgroup-strided loops)
    if (!c.valid) {
        c.commit_image();
        return;
    }
    float vq[7], vqd[6], vbp[NT_BODY_PARAM_FLOATS], vjp[NT_JOINT_PARAM_FLOATS], vdp[NT_DOF_PARAM_FLOATS], vsp[NT_SHAPE_PARAM_FLOATS];
    float vg[3] = {0.0f, 0.0f, 0.0f}, vcf = 0.0f, vctq = 0.0f, vctqd = 0.0f;
    int flags = 0;
    if (state) {
        first_load(c, state->body_q, nb, vq);
        first_load(c, state->body_qd, nb, vqd);
    }
    if constexpr (!UNI) {
        first_load(c, m.body_param, nb, vbp);
        if (c.slot < nb) flags = m.body_flags[c.slot];
        first_load(c, m.joint_param, m.nj, vjp);
        first_load(c, m.dof_param, m.nd, vdp);
        first_load(c, m.shape_param, m.ns, vsp);
    }
    if (c.slot == 0) {  // (one item of three components: tiny models run with fewer than three slot-threads per environment)
#pragma unroll
        for (int k = 0; k < 3; ++k) vg[k] = m.gravity[(size_t)k * c.ES + c.env];
    }
    if (with_control) {
        if (c.slot < m.nd) { vcf = c.a.c.joint_f[c.g(0, m.nd, c.slot)]; vctqd = c.a.c.joint_target_qd[c.g(0, m.nd, c.slot)]; }
        if (c.slot < m.ntq) vctq = c.a.c.joint_target_q[c.g(0, m.ntq, c.slot)];
    }
    // ---- writes (first a deferred tile image: its loads left before the ones above)
    c.commit_image();
    if (state) {
        first_store(c, c.L.bq, nb, vq);
        first_store(c, c.L.bqd, nb, vqd);
    }
    if constexpr (!UNI) {
#pragma unroll
        for (int k = 0; k < NT_BODY_PARAM_FLOATS; ++k) vbp[k] = effective_body_param(k, flags, vbp[k]);
        first_store(c, c.L.bp, nb, vbp);
        first_store(c, c.L.jp, m.nj, vjp);
        first_store(c, c.L.dp, m.nd, vdp);
        first_store(c, c.L.sp, m.ns, vsp);
    }
    if (c.slot == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) c.l(c.L.grav, k, 1, 0) = vg[k];
    }
    if (with_control) {
        if (c.slot < m.nd) { c.l(c.L.cf, 0, m.nd, c.slot) = vcf; c.l(c.L.ctqd, 0, m.nd, c.slot) = vctqd; }
        if (c.slot < m.ntq) c.l(c.L.ctq, 0, m.ntq, c.slot) = vctq;
    }
    // ---- items beyond the first trip
    const int rest = c.slot + c.nslot;
    if (state) {
        stage_rows(c, c.L.bq, state->body_q, 7, nb, rest);
        stage_rows(c, c.L.bqd, state->body_qd, 6, nb, rest);
    }
    if constexpr (!UNI) {
        stage_body_params<1>(c, rest);  // (one component at a time: a batch of eight here is unmeasured in the rollout kernels)
        stage_rows(c, c.L.jp, m.joint_param, NT_JOINT_PARAM_FLOATS, m.nj, rest);
        stage_rows(c, c.L.dp, m.dof_param, NT_DOF_PARAM_FLOATS, m.nd, rest);
        stage_rows(c, c.L.sp, m.shape_param, NT_SHAPE_PARAM_FLOATS, m.ns, rest);
    }
    if (with_control) {
        stage_rows(c, c.L.cf, c.a.c.joint_f, 1, m.nd, rest);
        stage_rows(c, c.L.ctq, c.a.c.joint_target_q, 1, m.ntq, rest);
        stage_rows(c, c.L.ctqd, c.a.c.joint_target_qd, 1, m.nd, rest);
    }
}
