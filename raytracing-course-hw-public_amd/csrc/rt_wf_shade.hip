// rt_wf_shade.hip — wf_shade, the shading stage of the wavefront pipeline (rt_wavefront.hip: the pipeline and its scheduler): one shade()
// level per closest hit, survivors compacted into the next ray queue, with the next bounce's sort keys where the scheduler asks for them.
#include "rt_dev_shade.h"
#include "rt_dev_stack.h"
#include "rt_kernels.h"
#include "rt_ray_key.h"
#include "rt_wf_records.h"

namespace {

#ifndef RT_SHADE_WAVES_PER_SIMD
#define RT_SHADE_WAVES_PER_SIMD 4
#endif
#ifndef RT_SHADE_LDS_DEPTH
#define RT_SHADE_LDS_DEPTH 4 /* only the light-BVH traversal of bvh_mix_dist::pdf uses a stack in wf_shade */
#endif

// ------------------------------------------------------------------------------------------------ shade
// LIGHTS_LDS: the light BVH (inner nodes, triangles, aux) is small enough (DevBvh::lds_inner) to be staged in LDS once per
// block; bvh_mix_dist's sample and pdf then read it there: a dozen dependent L1 round trips per hit become LDS reads.
template <bool STATS, bool LIGHTS_LDS, int ENV> __global__ __launch_bounds__(256, RT_SHADE_WAVES_PER_SIMD) void wf_shade(const DevScene S, const WfLaunch L) {
    __shared__ float s_lin[256];
    __shared__ float s_gam[256];
    __shared__ uint32_t s_stack[STACK_LDS_DWORDS(RT_SHADE_LDS_DEPTH, 3)];
    __shared__ float4 s_lights[LIGHTS_LDS ? RT_SHADE_LIGHTS_F4 : 1];
    __shared__ uint2 s_perm[4][256]; // per wave: (queue position, queue slot) of its 256 positions, sorted by sampler class
    LightTabs LT = light_tabs_global(S);
    if (LIGHTS_LDS) {
        const uint32_t n_node_f4 = 4u * (S.lights.lds_inner - 1u), n_tri_f4 = 3u * S.lights.n_tris;
        for (uint32_t i = threadIdx.x; i < n_node_f4; i += blockDim.x)
            s_lights[i] = LT.nodes[i];
        for (uint32_t i = threadIdx.x; i < n_tri_f4; i += blockDim.x)
            s_lights[n_node_f4 + i] = LT.tris[i];
        for (uint32_t i = threadIdx.x; i < S.lights.n_tris; i += blockDim.x)
            s_lights[n_node_f4 + n_tri_f4 + i] = LT.aux[i];
        LT = LightTabs{s_lights, s_lights + n_node_f4, s_lights + n_node_f4 + n_tri_f4};
    }
    s_lin[threadIdx.x] = S.lut_linear[threadIdx.x];
    s_gam[threadIdx.x] = S.lut_gamma[threadIdx.x];
    __syncthreads();
    LaneStats<STATS> st;
    RT_DECLARE_STACK(stk, RT_SHADE_LDS_DEPTH, s_stack);
    const bool has_lights = S.lights.n_tris != 0; // raytracer.h:449-453
    const uint32_t n_in = L.counters[WF_CNT_IN];
    const uint32_t n_slots = (n_in + 63u) >> 6; // wave slots of this launch: positions 64w .. 64w+63
    // one shade() level for the hit at queue position jq (the ray in queue slot j), as the lanes of one wave; `wave_slot` is the wave slot
    // (64 positions) this trip stands for: survivors go to the sub-queue of that slot (rt_device_types.h, WF_STRIPES)
    auto shade_wave = [&](const uint32_t jq, const uint32_t j, const uint32_t wave_slot) {
        const bool active = jq < n_in;
        bool survive = false;
        WfPacked next;
        uint32_t next_key = 0u; // the ray-order key of `next`, made only when the next bounce may be sorted (WfLaunch::emit_keys)
        if (active) {
            const Hit h = wf_load_hit(L.hits + jq); // first: the attributes and texel addresses hang on the hit alone, and loads return in order
            const WfHead in = wf_load_head(L.paths_in + j); // its class bits chose this lane (below); nothing here reads them
            Rng<RT_RNG_DEVICE> rng = wf_load_rng(L.paths_in + j);
            const uint32_t path = in.id;
            uint32_t depth_left = in.depth_left, nb = in.nb;
            if (h.k != RT_NONE)
                depth_left -= 1; // shade(..., max_depth - 1)
            const ShadeResult sr = shade_hit<Rng<RT_RNG_DEVICE>, STATS, ENV>(S, LT, h, in.o, in.d, rng, has_lights, stk, s_lin, s_gam, st);
            bool terminal = sr.terminal;
            V3 term = sr.term;
            if (sr.push) // emission + trace_ray(...) * scl (raytracer.h:588-590), folded when the path ends
                wf_store_fold(L, nb++, path, sr.emission, sr.scl);
            if (!terminal && depth_left == 0) { // trace_ray(..., 0) returns (0,0,0) without casting (:596-598)
                terminal = true;
                term = mk(0, 0, 0);
            }
            if (terminal) {
                // The pending shade() frames are folded by wf_fold after the last bounce, not here: at any bounce only about a
                // quarter of a wave's paths end, each with its own number of frames, so the unwind ran at 16 of 64 lanes behind
                // dependent loads (14 % of this kernel's cycles). Leave the innermost value and the frame count.
                L.sample_out[path] = RtF4{term.x, term.y, term.z, __uint_as_float(nb)};
                st.sample();
            } else {
                survive = true;
                st.cast();
                next = wf_pack(sr.nro, sr.nrd, path, next_shade_class<ENV == ENV_FLOAT_DIST>(rng, has_lights), depth_left, nb, rng.g);
                if (L.emit_keys)
                    next_key = rt_ray_order_key(sr.nro.x, sr.nro.y, sr.nro.z, sr.nrd.x, sr.nrd.y, sr.nrd.z, S.bounds_lo, S.bounds_inv);
            }
        }
        // compact the survivors of this wave into the next queue: ballot + prefix sum, one atomic per wave, on the counter of
        // the sub-queue this wave slot belongs to (rt_device_types.h, WF_STRIPES)
        const unsigned long long m = __ballot(survive);
        if (m != 0ull) {
            const uint32_t rank = lane_rank(m);
            uint32_t obase = 0;
            const int leader = __ffsll((long long)m) - 1;
            const uint32_t stripe = /* the wave's own slot: a sub-queue holds what ITS slots can emit */ (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_slot) % WF_STRIPES;
            if ((int)(threadIdx.x & 63u) == leader)
                obase = wf_stripe_base(stripe, n_slots) + atomicAdd(L.stripes + stripe * WF_STRIPE_WORDS, (uint32_t)__popcll(m));
            obase = __shfl(obase, leader);
            if (survive) {
                const uint32_t p = obase + rank;
                wf_store_path(L.paths_out + p, next);
                if (L.emit_keys) { // the sort's input, at the ray's physical slot: nobody reads the record again to make it
                    L.sort_keys[0][p] = next_key;
                    L.sort_vals[0][p] = wf_word(p, wf_word_class(__float_as_uint(next.p1.z))); // the class of the path word rides along above the slot (WfLaunch::order)
                }
            }
        }
    };
    // Which of shade()'s three samplers a hit runs is decided by its path's next draws alone (alpha coin, technique coin, mix pick:
    // raytracer.h:559,565,386): whoever wrote the path record left that class in the top bits of its path word, and the ray-order pass carried it along
    // in the top bits of `order`. A WAVE takes 256 queue positions at a time and hands them to its lanes sorted by class (a counting sort
    // over indices through the wave's own LDS window, before anything else is loaded, no block barrier): of its four trips one or two run
    // a single sampler and the others two instead of all three, and the rays aimed at a light walk the light BVH of bvh_mix_dist::pdf
    // side by side. Every wave still gets every class, so the waves of a block stay balanced. Which lane shades a hit changes no result.
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    // A queue too short to give every wave of the grid such a window is shaded 64 positions at a time (more waves, no reordering), and so
    // is one no sort ran over (primary rays; RT_SORT_OFF; the wide tree of a cache-resident scene): fetching the class from the records
    // ahead of the shading costs that kernel 6 % (measured, profiles/r04_variants.txt item 11); in the sort's payload it is free.
    const uint32_t win = (L.order_classed && n_in >= gridDim.x * 1024u) ? 256u : 64u;
    for (uint32_t wbase = (blockIdx.x * 4u + wv) * win; wbase < n_in; wbase += gridDim.x * 4u * win) { // wave-uniform
        uint32_t slot_of[4], cls[4], before[3] = {0u, 0u, 0u}, within[4];
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) {
            const uint32_t jq = wbase + 64u * q + lane;
            slot_of[q] = jq, cls[q] = 3u; // class 3: the positions behind the queue's (or the window's) end
            if (64u * q < win && jq < n_in) {
                const uint32_t v = wf_order_word(L, jq);
                slot_of[q] = wf_word_slot(v), cls[q] = wf_word_class(v);
            }
        }
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) { // position inside the class: the class's members in earlier quarters, then in lower lanes
            const unsigned long long b0 = __ballot(cls[q] == 0u), b1 = __ballot(cls[q] == 1u), b2 = __ballot(cls[q] == 2u);
            const unsigned long long mine = cls[q] == 0u ? b0 : cls[q] == 1u ? b1 : cls[q] == 2u ? b2 : ~(b0 | b1 | b2);
            const uint32_t seen = cls[q] == 0u ? before[0] : cls[q] == 1u ? before[1] : cls[q] == 2u ? before[2] : 64u * q - before[0] - before[1] - before[2];
            within[q] = seen + lane_rank(mine);
            before[0] += (uint32_t)__popcll(b0), before[1] += (uint32_t)__popcll(b1), before[2] += (uint32_t)__popcll(b2);
        }
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) {
            const uint32_t start = cls[q] == 0u ? 0u : cls[q] == 1u ? before[0] : cls[q] == 2u ? before[0] + before[1] : before[0] + before[1] + before[2];
            s_perm[wv][start + within[q]] = make_uint2(wbase + 64u * q + lane, slot_of[q]);
        }
        __builtin_amdgcn_wave_barrier(); // the wave's LDS operations complete in order: its reads below see the writes above
        const uint32_t n_here = n_in - wbase < win ? n_in - wbase : win;
        for (uint32_t sub = 0; 64u * sub < n_here; ++sub) {
            const uint2 pj = s_perm[wv][64u * sub + lane];
            shade_wave(pj.x, pj.y, (wbase >> 6) + sub);
        }
        __builtin_amdgcn_wave_barrier();
    }
    st.flush(L.stats);
}

} // namespace

namespace rt {

// The instantiation a scene shades with, over `blocks` blocks (grid-stride).
// ENV: the scene has an environment map (DevScene::bg_tex): the miss branch looks it up (scene.h:83-89); those instantiations read the
// light tables from global memory (LIGHTS_LDS only saves latency), so a scene without one never pays for the lookup's registers
// A float map (rt_set_environment, DevScene::env) takes the texture's place: ENV_FLOAT, or ENV_FLOAT_DIST when it has a distribution
// and mix_dist samples it. A scene without one launches what it always launched.
hipError_t launch_shade(const DevScene &S, const WfLaunch &L, bool stats, uint32_t blocks, hipStream_t stream) {
    const bool fenv = S.env.texels != nullptr;
    const bool env = fenv ? S.env.marg != nullptr : S.bg_tex >= 0;
    const bool lights_lds = S.lights.lds_inner != 0u && !env && !fenv;
    return with_bools([&](auto ST, auto LDS, auto FENV, auto ENV) {
        constexpr int KIND = FENV ? (ENV ? ENV_FLOAT_DIST : ENV_FLOAT) : (ENV ? ENV_TEX8 : ENV_NONE);
        if constexpr (LDS && KIND != ENV_NONE) // never chosen (above), never instantiated
            return hipErrorInvalidValue;
        else
            return RT_LAUNCH_CHECKED((wf_shade<ST, LDS, KIND>), dim3(blocks), dim3(256), 0, stream, S, L);
    }, stats, lights_lds, fenv, env);
}

} // namespace rt
