// The body of din_walk_bwd_kernel<GLOBAL_DX> and of din_walk_bwd_nodx_kernel (din_walk.hip includes it inside both, with GLOBAL_DX and NO_DX
// in scope): one text, so the two scatter kernels compile to what they were before the scatter-free form existed.
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int cells = p.hp * p.wp;
    float* tile = smem;                       // P
    float* dtile = tile + cells * CH;         // dP (LDS mode only)
    float* off_s = dtile + (GLOBAL_DX ? 0 : cells * CH);        // t*n*2*k2 offsets
    float* a_s = off_s + p.t * p.n * 2 * p.k2; // t*n*k2 saved relation weights
    const int nchunks = (p.c + CH - 1) / CH;
    const int ngroups = p.ngroups;
    const int grp = blockIdx.x % ngroups, bc = blockIdx.x / ngroups;
    const int b = bc / nchunks, chunk = bc % nchunks, c0 = chunk * CH;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nb = clip_n(p, b), wpc = nb + 2 * p.pl;
    stage_tile(p, p.x, b, c0, tile);
    stage_offsets(p, b, off_s);
    for (int i = threadIdx.x; i < p.t * p.n * p.k2; i += (int)blockDim.x) a_s[i] = p.a[(int64_t)b * p.t * p.n * p.k2 + i];
    if (!GLOBAL_DX)
        for (int i = threadIdx.x; i < cells * CH; i += (int)blockDim.x) dtile[i] = 0.f;
    __syncthreads();
    const bool cok = c0 + lane < p.c;
    // feature-gradient scatter of one corner: LDS tile, or dx itself when the tile does not fit
    auto scatter = [&](int cy, int cx, float v) {
        if (NO_DX) return;
        if (!GLOBAL_DX) { atomicAdd(&dtile[(cy * p.wp + cx) * CH + lane], v); return; }
        const int tt2 = cy - p.pt, nn2 = cx - p.pl;
        if (cok && tt2 >= 0 && tt2 < p.t && nn2 >= 0 && nn2 < nb && v != 0.f)
            atomicAdd(&p.dx[((int64_t)(b * p.t + tt2) * p.n + nn2) * p.c + c0 + lane], v);
    };
    // per-chunk partial sums, plain stores (each (chunk, position, k) is written exactly once): scratch[chunk][ d_off [b,t,n,2k2] | d_a [b,t,n,k2] ];
    // din_walk_bwd_finish_kernel adds the chunks in a fixed order
    float* d_off = p.scratch + (int64_t)chunk * p.b * p.t * p.n * 3 * p.k2;
    float* d_a = d_off + (int64_t)p.b * p.t * p.n * 2 * p.k2;
    for (int pos = grp * WALK_BWD_WAVES + w; pos < p.t * p.n; pos += ngroups * WALK_BWD_WAVES)
    if (pos % p.n >= nb) {                                // padding actor: no gradient (the finish kernel sums every chunk's slot)
        const int64_t gpos = (int64_t)b * p.t * p.n + pos;
        for (int j = lane; j < 3 * p.k2; j += 64) {
            if (j < 2 * p.k2) d_off[gpos * 2 * p.k2 + j] = 0.f; else d_a[gpos * p.k2 + (j - 2 * p.k2)] = 0.f;
        }
    } else {
        int tt = pos / p.n, nn = pos - tt * p.n;
        const int64_t gpos = (int64_t)b * p.t * p.n + pos;
        const float* pr = off_s + pos * 2 * p.k2;
        const float g = cok ? p.gz[gpos * p.c + c0 + lane] : 0.f;
        for (int k = 0; k < p.k2; ++k) {
            const float ak = a_s[pos * p.k2 + k];
            if (p.plain) {
                const int r = k / p.kw, s2 = k - r * p.kw;
                const int cy = p.pt + tt + p.ky0 + r * p.ratio, cx = p.pl + nn + p.kx0 + s2 * p.ratio;
                const float sk = tile[(cy * p.wp + cx) * CH + lane];
                scatter(cy, cx, ak * g);
                const float d_s = wave_sum(g * sk);
                if (lane == 0) { d_off[gpos * 2 * p.k2 + k] = 0.f; d_off[gpos * 2 * p.k2 + p.k2 + k] = 0.f; d_a[gpos * p.k2 + k] = d_s; }
                continue;
            }
            Corner c = corners(p, wpc, tt, nn, k, pr[k], pr[p.k2 + k]);
            float wy_l = coef(c.py, c.ly), wy_r = coef(c.py, c.ry), wx_l = coef(c.px, c.lx), wx_r = coef(c.px, c.rx);
            const int i_lt = (c.ly * p.wp + c.lx) * CH + lane, i_rb = (c.ry * p.wp + c.rx) * CH + lane;
            const int i_lb = (c.ry * p.wp + c.lx) * CH + lane, i_rt = (c.ly * p.wp + c.rx) * CH + lane;
            float v_lt = tile[i_lt], v_rb = tile[i_rb], v_lb = tile[i_lb], v_rt = tile[i_rt];
            float sk = v_lt * (wy_l * wx_l) + v_rb * (wy_r * wx_r) + v_lb * (wy_r * wx_l) + v_rt * (wy_l * wx_r);
            // feature gradient: scatter-add a_k * w_corner * gz into the padded tile (LDS atomics; waves may collide)
            const float ag = ak * g;
            scatter(c.ly, c.lx, ag * (wy_l * wx_l));
            scatter(c.ry, c.rx, ag * (wy_r * wx_r));
            scatter(c.ry, c.lx, ag * (wy_r * wx_l));
            scatter(c.ly, c.rx, ag * (wy_l * wx_r));
            // per-corner <gz, P_corner> and <gz, S_k> over this channel chunk
            float d_s = wave_sum(g * sk);
            float d_lt = wave_sum(g * v_lt), d_rb = wave_sum(g * v_rb), d_lb = wave_sum(g * v_lb), d_rt = wave_sum(g * v_rt);
            if (lane == 0) {
                // d/d py of (1-|py-cy|) = -sign(py-cy); clamp passes gradient on the closed interval (Q8, Q9)
                const float my = (c.py0 >= 0.f && c.py0 <= (float)(p.phy >= 0 ? p.phy : (p.ihy >= 0 ? p.ihy : p.hp - 1))) ? 1.f : 0.f;
                const float mx = (c.px0 >= 0.f && c.px0 <= (float)(p.phx >= 0 ? p.phx : (p.ihx >= 0 ? p.ihx : wpc - 1))) ? 1.f : 0.f;
                const float sy_l = -sgn(c.py - (float)c.ly), sy_r = -sgn(c.py - (float)c.ry);
                const float sx_l = -sgn(c.px - (float)c.lx), sx_r = -sgn(c.px - (float)c.rx);
                float doy = d_lt * sy_l * wx_l + d_rb * sy_r * wx_r + d_lb * sy_r * wx_l + d_rt * sy_l * wx_r;
                float dox = d_lt * wy_l * sx_l + d_rb * wy_r * sx_r + d_lb * wy_r * sx_l + d_rt * wy_l * sx_r;
                d_off[gpos * 2 * p.k2 + k] = my * ak * doy;
                d_off[gpos * 2 * p.k2 + p.k2 + k] = mx * ak * dox;
                d_a[gpos * p.k2 + k] = d_s;
            }
        }
    }
    if (GLOBAL_DX) return;
    __syncthreads();
    // un-pad and add this group's share: dx[b,t,n,c] += dP[pt+t][pl+n][c]
    for (int q = w; q < p.t * p.n; q += WALK_BWD_WAVES) {
        int tt = q / p.n, nn = q - tt * p.n;
        if (nn >= nb) continue;                            // cells beyond the clip's grid are zero padding: their gradient is dropped
        const float v = dtile[((p.pt + tt) * p.wp + p.pl + nn) * CH + lane];
        if (cok && v != 0.f) atomicAdd(&p.dx[((int64_t)b * p.t * p.n + q) * p.c + c0 + lane], v);
    }
