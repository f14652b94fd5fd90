"""The (configuration, rows) cases of tests/test_gpu_rawstate_rows.py, importable without a GPU (tests/test_rawtrain_scratch_host.py
sizes every one of them on the host before any of them runs on a device).

The forms are read from the selection code, with Ns the rows of the call:
  st_tn   (simtrain.hpp, reduce_plan.hpp)  Ns <= 1024: k_gemm_tn4;  Ns >= 4096 and M, Nc >= 64 and lda, ldb, M, Nc multiples of 4:
          k_gemm_tn_t128 + k_reduce_chunks4 (on this handle min(ceil(256 / tiles), 64, ceil(Ns / 512)) chunks);  else k_gemm_tn in
          ceil(Ns / 512) chunks of 512 rows + k_reduce_chunks
  st_cs   ceil(Ns / 512) chunks: one writes the destination, more go through cx.part + k_reduce_chunks
  st_back Ns <= 2048 and ceil(Ns / 128) * ceil(Kin / 64) < 512: k_gemm_nt;  else k_transpose into cx.wt + launch_gemm_f32
  launch_gemm_f32 (gemm.hip), an [M, K] x [K, N] product: ceil(M / 128) * ceil(N / 64) < 96 or N <= 32: k_gemm_small;  else M >= 2048,
          N >= 96, K >= 32 and K, N, lda, ldw multiples of 4: k_gemm_f32_t128;  else k_gemm_f32
The forward is dense_w1 [Dn, U] (lda = Dn from unpacked arrays, REC from records), dense_w2 [U, U], ctx_w [F, 256] and the head
[256, AE]; a transposed st_back is a forward GEMM with N = Kin."""

BASE = dict(maxlen=16, seq_num=2, category_feature_num=21, emb_size=64, hidden_units=128, dense_feature_num=432, action_size=284,
            category_hash_size=3000)                                    # F 320, AE 285, REC 488
ODD = dict(maxlen=5, seq_num=3, category_feature_num=3, emb_size=72, hidden_units=90, dense_feature_num=61, action_size=100,
           category_hash_size=500)                                      # F 378, AE 101, REC 80: no width a multiple of 4 but REC
U512 = dict(maxlen=4, seq_num=1, category_feature_num=2, emb_size=32, hidden_units=512, dense_feature_num=61, action_size=40,
            category_hash_size=500)                                     # F 576, AE 41, REC 68; U * U = 262144 > F * 256 = 147456
U512_D64 = dict(U512, dense_feature_num=64)                             # REC 72

CASES = {
    # gradients: all four k_gemm_tn in chunks of 512 / 512 / 6 rows + k_reduce_chunks; the four st_cs through 3 partials in cx.part
    # st_back: all three k_gemm_nt (9 row tiles x at most 5 column tiles)
    # forward: all four k_gemm_small (9 x 2, 9 x 4, 9 x 5 workgroups of the 128 x 64 tiling < 96)
    'base_n1030': (BASE, 1030),
    # gradients: k_gemm_tn in 5 chunks, the last of 52 rows; st_cs 5 partials
    # st_back: all three k_transpose ([256, 285], [320, 256], [128, 128]) + a forward GEMM, k_gemm_small (17 x 4, 17 x 5, 17 x 2 < 96)
    # forward: all four k_gemm_small (17 x 2, 17 x 4, 17 x 5 < 96) - from unpacked arrays and from records alike
    'base_n2100': (BASE, 2100),
    # gradients: k_gemm_tn_t128 in 9 chunks of 464 rows + k_reduce_chunks4 for ctx_w (320 x 256, 6 tiles), dense_w2 (128 x 128, ldb 320)
    #            and dense_w1 (432 x 128, lda 432 or REC 488); head_w (Nc 285) k_gemm_tn in 9 chunks; st_cs 9 partials
    # st_back: transposes; the GEMMs: head -> ctx (N 256, K 285) k_gemm_f32 (K odd), ctx -> feat (N 320, K 256) k_gemm_f32_t128,
    #          dense_w2 (N 128: 33 x 2 workgroups) k_gemm_small
    # forward: dense_w1 and dense_w2 k_gemm_small (33 x 2), ctx_w k_gemm_f32_t128 (33 x 4, lda 320), head k_gemm_f32 (N 285)
    'base_n4100': (BASE, 4100),
    # gradients: nothing aligned - all four k_gemm_tn in 9 chunks; st_cs 9 partials
    # st_back: transposes of [256, 101], [378, 256], [90, 90]; the GEMMs: N 256 k_gemm_f32 (K 101), N 378 k_gemm_f32 (N and ldw 378),
    #          N 90 k_gemm_small (33 x 2)
    # forward: dense_w1 / dense_w2 (N 90) k_gemm_small, ctx_w (K 378, lda 378) k_gemm_f32, head (N 101: 33 x 2) k_gemm_small
    'odd_n4100': (ODD, 4100),
    # the configuration whose dense_w2 partials (5 x 262144 floats) and transpose (262144) outgrew the scratch sized without U * U
    # gradients: k_gemm_tn in 5 chunks (dense_w2: 256 tiles); st_cs 5 partials
    # st_back: transposes of [256, 41], [576, 256], [512, 512]; the GEMMs: N 256 k_gemm_small (17 x 4), N 576 k_gemm_f32_t128
    #          (17 x 9, K 256), N 512 k_gemm_f32_t128 (17 x 8, K 512, lda F = 576)
    # forward: dense_w1 k_gemm_f32 (17 x 8 workgroups, K 61), dense_w2 k_gemm_f32_t128 (K 512), ctx_w and head k_gemm_small
    'u512_n2100': (U512, 2100),
    # as u512_n2100 with Dn = 64: dense_w1 takes k_gemm_f32_t128 too, with lda = 64 from unpacked arrays and lda = REC = 72 from
    # records - the one place a forward from records and a forward from arrays run the LDS-tiled GEMM on differently strided rows
    'u512d64_n2100': (U512_D64, 2100),
}
DQN_CASES = ('base_n1030', 'base_n4100', 'odd_n4100', 'u512_n2100')
RECORD_CASES = ('base_n2100', 'u512d64_n2100')          # greedy from arrays against a* from records, bit for bit


def dims(cfg):
    """-> (F, AE, REC)"""
    used = cfg['dense_feature_num'] + cfg['category_feature_num'] + cfg['seq_num'] * cfg['maxlen']
    return cfg['seq_num'] * cfg['emb_size'] + cfg['hidden_units'] + cfg['emb_size'], cfg['action_size'] + 1, (used + 3) // 4 * 4
