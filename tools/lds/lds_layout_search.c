// Exhaustive LDS bank-conflict count for the multislice kernel's field image (tools/lds/README in tools/README.md).
// Element (y, x) of the P x P complex field lives at complex index  y*Q + (x / R2)*PA + (x % R2)*PB.
// Access patterns = the four line roles of adm_multislice.hip (row/column x pass-1/pass-2), each as ds_read_b64
// (two groups of 32 lanes, 64 banks of 4 B: complex index distinct mod 32) and ds_write_b64 (four groups of 16 lanes,
// 32 banks: complex index distinct mod 16) -- MI355X_MICROARCH.md, LDS table.  Score = LDS-array cycles per 2-D pass set
// summed over all waves; the conflict-free floor is printed first.
// Merged forms (same table): where the compiler pairs elements k, k+1 of a line into ONE ds_read2_b64 / ds_write2_b64, the
// instruction is two accesses of four groups of 16 lanes each over 32 banks (complex index distinct mod 16): 8 array cycles
// conflict-free for the read -- twice what two ds_read_b64 cost -- and ~13 for the write (two ds_write_b64: ~12).  Which line
// roles are merged is what tools/isa_lds_forms.py shows for the build; arguments 6 and 7 are bit masks over the roles
// (1 row pass 1, 2 row pass 2, 4 column pass 1, 8 column pass 2) for reads and writes.  Default = the shipped build:
// adm_multislice.hip is compiled without the backend's load/store merging, which leaves only the stride-1 role of
// P = 72 paired (mask 1; its pairs come from the IR-level vectorizer), nothing at the other sizes.  The build before that
// merged every role whose pair fits the 8-bit offsets of the merged forms: masks 11 11 (all but column pass 1).
// build: gcc -O2 -o lds_layout_search lds_layout_search.c ; run: ./lds_layout_search N R1 R2 [Qmax] [time_model] [rd_mask] [wr_mask]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
static int N, R1, R2, G, LPW, NW, TIME_MODEL, RD_MASK, WR_MASK;
static int posx(int x, int PA, int PB) { return (x / R2) * PA + (x % R2) * PB; }
static int group_cycles(const int* e, const int* act, int lo, int hi, int mod) {
    int cnt[64]; int seen[64][64]; int ns[64];
    memset(ns, 0, sizeof ns);
    for (int l = lo; l < hi; ++l) {
        if (!act[l]) continue;
        int b = ((e[l] % mod) + mod) % mod, dup = 0;
        for (int j = 0; j < ns[b]; ++j) if (seen[b][j] == e[l]) dup = 1;   // same address broadcasts
        if (!dup) seen[b][ns[b]++] = e[l];
    }
    int m = 0; for (int b = 0; b < mod; ++b) if (ns[b] > m) m = ns[b];
    (void)cnt; return m ? m : 0;
}
static long score(int PA, int PB, int Q, long* rd_out, long* wr_out) {
    long rd = 0, wr = 0;
    for (int w = 0; w < NW; ++w)
        for (int pat = 0; pat < 4; ++pat) {
            int R = (pat == 0 || pat == 2) ? R1 : R2;
            // uses per propagation (adm_multislice.hip: convolve): row pass 1 once, row pass 2 and column pass 1 twice, column
            // pass 2 once -- each as a load and as a store
            const int uses = (pat == 1 || pat == 2) ? 2 : 1;
            int g16[16], g32[16];       // per element k: array cycles as four 16-lane groups / as two 32-lane groups
            for (int k = 0; k < R; ++k) {
                int e[64], act[64];
                for (int l = 0; l < 64; ++l) {
                    int li = l / G, t = l % G, line = w * LPW + li;
                    act[l] = (li < LPW) && (line < N) && ((pat == 0 || pat == 2) ? (t < R2) : (t < R1));
                    if (!act[l]) { e[l] = 0; continue; }
                    int idx = (pat == 0 || pat == 2) ? (k * R2 + t) : (t * R2 + k);   // element index along the line
                    e[l] = (pat < 2) ? line * Q + posx(idx, PA, PB) : idx * Q + posx(line, PA, PB);
                }
                g32[k] = group_cycles(e, act, 0, 32, 32) + group_cycles(e, act, 32, 64, 32);
                g16[k] = 0;
                for (int g = 0; g < 4; ++g) g16[k] += group_cycles(e, act, 16 * g, 16 * g + 16, 16);
            }
            // MI355X_MICROARCH.md, LDS (TIME_MODEL): a ds_write_b64 holds the pipe for ~6 cycles whatever the array does (address +
            // data transfer), so its first two conflict cycles are free; a ds_read_b64 is 2 array cycles conflict-free; a
            // ds_read2_b64 8 and a ds_write2_b64 ~13
            const int rd_merged = (RD_MASK >> pat) & 1, wr_merged = (WR_MASK >> pat) & 1;
            for (int k = 0; k < R; ++k) {
                const int pair = k + 1 < R;
                if (rd_merged && pair) { int r_ = g16[k] + g16[k + 1]; if (TIME_MODEL && r_ < 8) r_ = 8; rd += uses * r_; }
                else { for (int j = k; j <= k + (rd_merged ? 0 : pair); ++j) { int r_ = g32[j]; if (TIME_MODEL && r_ < 2) r_ = 2; rd += uses * r_; } }
                if (wr_merged && pair) { int w_ = g16[k] + g16[k + 1]; if (TIME_MODEL && w_ < 13) w_ = 13; wr += uses * w_; }
                else { for (int j = k; j <= k + (wr_merged ? 0 : pair); ++j) { int w_ = g16[j]; if (TIME_MODEL && w_ < 6) w_ = 6; wr += uses * w_; } }
                if (pair) ++k;          // (elements k and k+1 are done, as one pair or as two singles)
            }
        }
    *rd_out = rd; *wr_out = wr; return rd + wr;
}
int main(int argc, char** argv) {
    N = argc > 1 ? atoi(argv[1]) : 72; R1 = argc > 2 ? atoi(argv[2]) : 8; R2 = argc > 3 ? atoi(argv[3]) : 9;
    int Qmax = argc > 4 ? atoi(argv[4]) : 128;
    TIME_MODEL = argc > 5 ? atoi(argv[5]) : 0;      // 1: instruction-time model and per-propagation use counts (round 4)
    RD_MASK = argc > 6 ? atoi(argv[6]) : (N == 72 ? 1 : 0);     // default: what the shipped build issues (see the head of this file)
    WR_MASK = argc > 7 ? atoi(argv[7]) : RD_MASK;
    G = R1 > R2 ? R1 : R2; LPW = 64 / G; NW = (N + LPW - 1) / LPW;
    long floor_rd = 0, floor_wr = 0;
    { long r, w; /* floor: count non-empty groups */
      for (int wv = 0; wv < NW; ++wv) for (int pat = 0; pat < 4; ++pat) { int R = (pat == 0 || pat == 2) ? R1 : R2; floor_rd += 2 * R; floor_wr += 4 * R; } (void)r; (void)w; }
    printf("N=%d R1=%d R2=%d G=%d LPW=%d waves=%d  floor(read,write)=(%ld,%ld)  merged roles: reads %d writes %d\n", N, R1, R2, G, LPW, NW, floor_rd, floor_wr,
           RD_MASK, WR_MASK);
    static char used[1 << 20];
    long best[64]; int bp[64][3]; int nb = 0;
    for (int Q = N; Q <= Qmax; ++Q)
        for (int PA = 1; PA <= Q; ++PA)
            for (int PB = 1; PB <= Q; ++PB) {
                // injective?
                int mx = 0, ok = 1;
                for (int x = 0; x < N; ++x) { int p = posx(x, PA, PB); if (p > mx) mx = p; }
                long fld = (long)(N - 1) * Q + mx + 1;
                if (fld >= (1 << 20)) continue;
                memset(used, 0, fld);
                for (int y = 0; y < N && ok; ++y) for (int x = 0; x < N; ++x) { int a = y * Q + posx(x, PA, PB); if (used[a]) { ok = 0; break; } used[a] = 1; }
                if (!ok) continue;
                long r, w, s = score(PA, PB, Q, &r, &w);
                printf("%ld %ld %ld Q=%d PA=%d PB=%d fld=%ld bytes=%ld\n", s, r, w, Q, PA, PB, fld, fld * 8);
            }
    (void)best; (void)bp; (void)nb;
    return 0;
}
