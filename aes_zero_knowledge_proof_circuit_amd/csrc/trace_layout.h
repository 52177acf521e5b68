// csrc/trace_layout.h -- byte layout of the per-proof AES "trace" buffer shared by the circuit compiler
// (which tags every allocated R1CS variable with the trace bit it equals) and the aes_trace HIP kernel
// (which fills the buffer from message + key).  One trace per chunk-proof:
//
//   [0,16)        key bytes
//   [16,192)      key-schedule words W_0..W_43, 4 bytes each, big-endian byte order (src/aes_circuit.rs:188-212)
//   [192,232)     SubWord(RotWord(W_{i-1})) bytes for i = 4,8,..,40
//   [232,272)     W_{i-4} ^ SubWord(..) (before the Rcon xor) for i = 4,8,..,40
//   [272, ...)    per ECB block, stride TR_BLOCK_STRIDE:
//       +0    message block (16)
//       +16   S_r, r = 0..10 : state after AddRoundKey of round r (S_10 = ciphertext block)     11 x 16
//       +192  SB_r, r = 1..10: state after SubBytes (before ShiftRows)                          10 x 16
//       +352  XT_r, r = 1..9 : xtime ("b") bytes of the ShiftRows output, src/aes_circuit.rs:366-389   9 x 16
//       +496  MP_r, r = 1..9 : for each output byte idx, the 4 partial values of its 5-term xor chain
//                              (src/aes_circuit.rs:391-426); partial 3 is the MixColumns output           9 x 64
//   CBC keys only, behind the nb blocks (cbc = TR_CBC(nb)); a block's "message block" stays the plaintext M_b and its S_0 is X_b ^ key:
//       cbc + 0          IV (16)
//       cbc + 16 + 16 b  X_b = M_b ^ C_{b-1}, C_{-1} = IV: what enters round 0 of block b    nb x 16
//   CTR keys only, at the same base (ctr = TR_CTR(nb)); a block's "message block" is M_b with zeros beyond the message's last byte and its S_0 is CTR_b ^ key:
//       ctr + 0               ICB, the initial counter block (16)
//       ctr + 16 + 48 b       CTR_b = ICB + b mod 2^128, big-endian (16)
//       ctr + 16 + 48 b + 16  K_b (16): the carries of CTR_{b-1} + 1.  Counter bit i (weight 2^i) is bit i % 8 of byte 15 - i / 8; bit i of K_b, in the same mapping,
//                             is the carry out of position i, i.e. 1 iff bits 0..i of CTR_{b-1} are all one.  K_0 = 0
//       ctr + 16 + 48 b + 32  C_b = M_b ^ S_10 (16), zero beyond the message's last byte
//   GCM keys only (message of L bytes, nb = ceil(L / 16); AAD of A bytes, na = ceil(A / 16); M = na + nb + 1 GHASH multiplications).  The trace holds nb + 2 AES
//   blocks: slots 0 .. nb - 1 are the message blocks under the counters iv || be32(b + 2), slot nb is H = AES_K(0^128), slot nb + 1 is AES_K(J_0), J_0 = iv || 00000001;
//   every slot's S_0 is its input ^ key, a message slot's "message block" is M_b with zeros beyond L.  Behind them, 16-byte aligned (gcm = TR_GCM(nb)):
//       gcm + 0                    iv (12) and 4 zero bytes
//       gcm + 16                   the AAD, zero-padded to 16 na bytes
//       gcm + 16 + 16 na           C_b = M_b ^ S_10, nb x 16, zero beyond L
//       then the V table (2048):   V_0 = H, V_{i+1} = V_i * alpha in GF(2^128); byte j of V_i at 128 j + i
//       then per multiplication m = 0 .. M - 1, stride TR_GCM_MUL_STRIDE (Y_m = X_m * H):
//           +0     X_m (16): X_0 = the first GHASH block, X_m = Y_{m-1} ^ block m (the AAD blocks, the C_b, last the length block be64(8 A) || be64(8 L))
//           +16    P_m (2048): p_{i,k} = x_i & V_i[k]; byte j of row i (x_i ? byte j of V_i : 0) at 128 j + i, so byte column j is 128 contiguous bytes
//           +2064  Q_m (128): byte k holds q_k = floor(sum_i p_{i,k} / 2) <= 64 in its bits 0..6
//           +2192  Y_m (16)
//       last                       the tag (16) = Y_{M-1} ^ S_10 of slot nb + 1
//   Bit k of a GHASH block (k = 0 is the coefficient of alpha^0) is bit 7 - k % 8 of byte k / 8 (SP 800-38D 6.3: the leftmost bit of byte 0 first).
#pragma once
#define TR_KEY 0
#define TR_KS_W 16
#define TR_KS_SUB 192
#define TR_KS_PRE 232
#define TR_BLOCK0 272
#define TR_BLOCK_STRIDE 1072
#define TR_BL_MSG 0
#define TR_BL_S 16
#define TR_BL_SB 192
#define TR_BL_XT 352
#define TR_BL_MP 496
#define TR_CBC(nb) (TR_BLOCK0 + (nb) * TR_BLOCK_STRIDE)
#define TR_CBC_IV 0
#define TR_CBC_X 16
#define TR_CTR(nb) TR_CBC(nb)
#define TR_CTR_ICB 0
#define TR_CTR_BLOCK0 16
#define TR_CTR_BLOCK_STRIDE 48
#define TR_CTR_BL_CTR 0
#define TR_CTR_BL_CARRY 16
#define TR_CTR_BL_CT 32
#define TR_CTR_BYTES(nb) (TR_CTR(nb) + TR_CTR_BLOCK0 + (nb) * TR_CTR_BLOCK_STRIDE)
#define TR_GCM(nb) TR_CBC((nb) + 2)
#define TR_GCM_IV 0
#define TR_GCM_AAD 16
#define TR_GCM_CT(na) (16 + 16 * (na))
#define TR_GCM_V(na, nb) (16 + 16 * (na) + 16 * (nb))
#define TR_GCM_MUL0(na, nb) (TR_GCM_V(na, nb) + 2048)
#define TR_GCM_MUL_STRIDE 2208
#define TR_GCM_MUL_X 0
#define TR_GCM_MUL_P 16
#define TR_GCM_MUL_Q 2064
#define TR_GCM_MUL_Y 2192
#define TR_GCM_MULS(na, nb) ((na) + (nb) + 1)
#define TR_GCM_TAG(na, nb) (TR_GCM_MUL0(na, nb) + TR_GCM_MULS(na, nb) * TR_GCM_MUL_STRIDE)
#define TR_GCM_BYTES(na, nb) (TR_GCM(nb) + TR_GCM_TAG(na, nb) + 16)
#define TR_SBOX_PER_BLOCK 160
#define TR_SBOX_KS 40

// ---- the same layout for every key size, nk = the key length in 32-bit words (4, 6, 8 for AES-128, -192, -256); Nr = nk + 6 rounds, 4 (Nr + 1) schedule words
// (FIPS-197 5.2).  The order of the parts is the one above; what moves is where each begins:
//   key (4 nk) | W_0 .. W_{4 Nr + 3} | SubWord bytes, 4 per instance | the word ahead of the Rcon xor, 4 per instance | blocks | the mode's tail
// A SubWord instance is every schedule index i >= nk with i % nk == 0 (SubWord(RotWord(W_{i-1})), then the Rcon xor) and, for nk = 8, also every i with i % 8 == 4
// (SubWord(W_{i-1}): no rotation and no Rcon, so that instance's "pre" word is W_i itself): 10, 8, 13 instances, numbered in the order of i (TRK_KS_INST_OF).
// A block slot is the message (16), S_0 .. S_Nr, SB_1 .. SB_Nr, XT_1 .. XT_{Nr-1}, MP_1 .. MP_{Nr-1}: 16 + 16 (Nr + 1) + 16 Nr + 16 (Nr - 1) + 64 (Nr - 1) = 112 Nr - 48 bytes.
// The CBC, CTR and GCM tails keep their inner layout (the TR_CBC_*, TR_CTR_*, TR_GCM_* offsets above) behind the blocks of the chosen stride; the GCM tail begins at the
// next multiple of 16 (at nk = 4 the blocks end on one).
#define TRK_NR(nk) ((nk) + 6)
#define TRK_KS_WORDS(nk) (4 * (TRK_NR(nk) + 1))
#define TRK_KEY_BYTES(nk) (4 * (nk))
#define TRK_KS_INST(nk) ((nk) == 8 ? 13 : (nk) == 6 ? 8 : 10)
#define TRK_KS_W(nk) TRK_KEY_BYTES(nk)
#define TRK_KS_SUB(nk) (TRK_KS_W(nk) + 4 * TRK_KS_WORDS(nk))
#define TRK_KS_PRE(nk) (TRK_KS_SUB(nk) + 4 * TRK_KS_INST(nk))
#define TRK_BLOCK0(nk) (TRK_KS_PRE(nk) + 4 * TRK_KS_INST(nk))
#define TRK_BLOCK_STRIDE(nk) (112 * TRK_NR(nk) - 48)
#define TRK_BL_S(nk) 16
#define TRK_BL_SB(nk) (TRK_BL_S(nk) + 16 * (TRK_NR(nk) + 1))
#define TRK_BL_XT(nk) (TRK_BL_SB(nk) + 16 * TRK_NR(nk))
#define TRK_BL_MP(nk) (TRK_BL_XT(nk) + 16 * (TRK_NR(nk) - 1))
#define TRK_BL_CT(nk) (TRK_BL_S(nk) + 16 * TRK_NR(nk))                 // S_Nr, the block's ciphertext, inside its slot
// the instance number of schedule index i (only for an i that is one): i / nk - 1, and for nk = 8 the i % 8 == 4 instances interleave
#define TRK_KS_INST_OF(nk, i) ((nk) == 8 ? (i) / 4 - 2 : (i) / (nk) - 1)
#define TRK_ECB_BYTES(nk, nb) (TRK_BLOCK0(nk) + (nb) * TRK_BLOCK_STRIDE(nk))
#define TRK_CBC(nk, nb) TRK_ECB_BYTES(nk, nb)
#define TRK_CBC_BYTES(nk, nb) (TRK_CBC(nk, nb) + TR_CBC_X + 16 * (nb))
#define TRK_CTR(nk, nb) TRK_CBC(nk, nb)
#define TRK_CTR_BYTES(nk, nb) (TRK_CTR(nk, nb) + TR_CTR_BLOCK0 + (nb) * TR_CTR_BLOCK_STRIDE)
#define TRK_GCM(nk, nb) ((TRK_CBC(nk, (nb) + 2) + 15) / 16 * 16)             // (the GHASH lanes store 16 bytes at a time: the blocks begin at 296 and 376 for nk = 6, 8, so 8 bytes of padding)
#define TRK_GCM_BYTES(nk, na, nb) (TRK_GCM(nk, nb) + TR_GCM_TAG(na, nb) + 16)
#define TRK_SBOX_PER_BLOCK(nk) (16 * TRK_NR(nk))
#define TRK_SBOX_KS(nk) (4 * TRK_KS_INST(nk))
// at nk = 4 every parametrised macro is the constant above: an AES-128 trace is byte for byte what it was
static_assert(TRK_KS_W(4) == TR_KS_W && TRK_KS_SUB(4) == TR_KS_SUB && TRK_KS_PRE(4) == TR_KS_PRE && TRK_BLOCK0(4) == TR_BLOCK0, "AES-128 key-schedule layout moved");
static_assert(TRK_BLOCK_STRIDE(4) == TR_BLOCK_STRIDE && TRK_BL_S(4) == TR_BL_S && TRK_BL_SB(4) == TR_BL_SB && TRK_BL_XT(4) == TR_BL_XT && TRK_BL_MP(4) == TR_BL_MP, "AES-128 block slot moved");
static_assert(TRK_BL_CT(4) == TR_BL_S + 160 && TRK_BL_MP(4) + 64 * (TRK_NR(4) - 1) == TR_BLOCK_STRIDE, "AES-128 block slot moved");
static_assert(TRK_CBC(4, 3) == TR_CBC(3) && TRK_CTR_BYTES(4, 3) == TR_CTR_BYTES(3) && TRK_GCM(4, 3) == TR_GCM(3) && TRK_GCM_BYTES(4, 2, 3) == TR_GCM_BYTES(2, 3), "AES-128 mode tails moved");
static_assert(TRK_SBOX_PER_BLOCK(4) == TR_SBOX_PER_BLOCK && TRK_SBOX_KS(4) == TR_SBOX_KS && TRK_KS_WORDS(4) == 44 && TRK_KS_INST_OF(4, 40) == 9, "AES-128 counts moved");
static_assert(TRK_BLOCK_STRIDE(6) == 1296 && TRK_BLOCK_STRIDE(8) == 1520 && TRK_KS_WORDS(6) == 52 && TRK_KS_WORDS(8) == 60, "block strides of AES-192 / -256");
static_assert(TRK_KS_INST_OF(6, 48) == 7 && TRK_KS_INST_OF(8, 8) == 0 && TRK_KS_INST_OF(8, 12) == 1 && TRK_KS_INST_OF(8, 56) == 12, "SubWord instance numbering");
static_assert(TRK_GCM(6, 1) % 16 == 0 && TRK_GCM(8, 1) % 16 == 0 && TRK_GCM(6, 1) == TRK_CBC(6, 3) + 8 && TRK_GCM(8, 2) == TRK_CBC(8, 4) + 8 && TRK_GCM_BYTES(6, 1, 2) % 16 == 0, "the GCM tail must stay 16-byte aligned");

// ---- key tags: a key synthesized with T = 1 or 2 key-tag blocks proves tag_t = AES_K(D_t), t < T, beside its mode's statement, D_t = "zkaes-keyta" || t ||
// 00 00 00 00.  The T tag slots lie BEHIND the mode's tail, so no offset above moves: `bytes` = the mode's own trace length (TRK_ECB_BYTES, TRK_CBC_BYTES, TRK_CTR_BYTES,
// TRK_GCM_BYTES), TRK_KT(bytes) = that length rounded up to 16 is slot 0, slot t follows at t block strides, and a slot has the ordinary block-slot layout: D_t in the
// "message" field, S_0 = D_t ^ key, ..., S_Nr = tag_t.  With T = 0 a trace is what it was.
#define TRK_KT(bytes) (((bytes) + 15) / 16 * 16)
#define TRK_KT_SLOT(nk, bytes, t) (TRK_KT(bytes) + (t) * TRK_BLOCK_STRIDE(nk))
#define TRK_KT_BYTES(nk, bytes, T) ((T) ? TRK_KT_SLOT(nk, bytes, T) : (bytes))
#define TRK_KT_D_PREFIX "zkaes-keyta"      // 11 bytes, none of them zero; byte 11 is t, bytes 12 .. 15 are zero
static_assert(TRK_KT_BYTES(4, TRK_ECB_BYTES(4, 1), 0) == TR_BLOCK0 + TR_BLOCK_STRIDE && TRK_KT_BYTES(8, TRK_CTR_BYTES(8, 2), 0) == TRK_CTR_BYTES(8, 2), "without key tags a trace keeps its length");
static_assert(TRK_KT(TRK_ECB_BYTES(4, 1)) == TRK_ECB_BYTES(4, 1) && TRK_KT(TRK_ECB_BYTES(6, 1)) == TRK_ECB_BYTES(6, 1) + 8 && TRK_KT(TRK_ECB_BYTES(8, 2)) == TRK_ECB_BYTES(8, 2) + 8, "tag slot 0 begins on the next multiple of 16");
static_assert(TRK_KT_SLOT(8, TRK_ECB_BYTES(8, 2), 1) == 3424 + 1520 && TRK_KT_BYTES(8, TRK_ECB_BYTES(8, 2), 2) == 3424 + 2 * 1520 && TRK_KT_BYTES(4, TRK_CTR_BYTES(4, 2), 1) == 2528 + 1072, "tag slots at the block stride");
static_assert(TRK_BLOCK_STRIDE(4) % 16 == 0 && TRK_BLOCK_STRIDE(6) % 16 == 0 && TRK_BLOCK_STRIDE(8) % 16 == 0 && TRK_KT_BYTES(6, TRK_GCM_BYTES(6, 1, 2), 1) % 16 == 0 && TRK_KT(TRK_GCM_BYTES(8, 1, 2)) == TRK_GCM_BYTES(8, 1, 2), "tagged traces are 16-byte multiples");
static_assert(sizeof(TRK_KT_D_PREFIX) == 12, "D_t = 11 prefix bytes, t, four zero bytes");

// ---- plaintext digests: a key synthesized with a digest kind D = 1 (chain) or 2 (final) also proves H_out = the SHA-256 compressions of its hidden message
// from H_in.  The digest region lies BEHIND the key-tag slots, so no offset above moves: `bytes` = the trace length with the tag slots (TRK_KT_BYTES), TRD(bytes) = that
// length rounded up to 16 is the region's base dg, and with D = 0 a trace is what it was.
//   dg + 0    H_in  (32): the eight words a proof's first compression starts from, in SHA-256's big-endian word serialisation (word k bit i = bit i % 8 of byte 4 k + 3 - i / 8)
//   dg + 32   H_out (32): the same for the last compression's feed-forward
//   dg + 64   one slot per compression, stride TRD_SLOT_STRIDE.  Every entry is a 32-bit word stored little-endian, so bit i of a word at `off` is (off + i / 8, i % 8):
//       +0     per schedule word t = 16 .. 63, 24 bytes: rotr7 ^ rotr18 of W_{t-15} | sigma_0(W_{t-15}) | rotr17 ^ rotr19 of W_{t-2} | sigma_1(W_{t-2}) | W_t | carry (2 bits)
//       +1152  per round t = 0 .. 63, 44 bytes: rotr6 ^ rotr11 of e | Sigma_1(e) | Ch | rotr2 ^ rotr13 of a | Sigma_0(a) | a ^ b | Maj | e' | a' | carry of e' (3 bits) |
//              carry of a' (3 bits)
//       +3968  the eight feed-forward sums (32), then their carries (8 words of one bit)
#define TRD(bytes) (((bytes) + 15) / 16 * 16)
#define TRD_HIN 0
#define TRD_HOUT 32
#define TRD_SLOT0 64
#define TRD_SCH 0
#define TRD_SCH_STRIDE 24
#define TRD_SCH_S0X 0
#define TRD_SCH_S0 4
#define TRD_SCH_S1X 8
#define TRD_SCH_S1 12
#define TRD_SCH_W 16
#define TRD_SCH_CARRY 20
#define TRD_RND (TRD_SCH + 48 * TRD_SCH_STRIDE)
#define TRD_RND_STRIDE 44
#define TRD_RND_S1X 0
#define TRD_RND_S1 4
#define TRD_RND_CH 8
#define TRD_RND_S0X 12
#define TRD_RND_S0 16
#define TRD_RND_AB 20
#define TRD_RND_MAJ 24
#define TRD_RND_E 28
#define TRD_RND_A 32
#define TRD_RND_CE 36
#define TRD_RND_CA 40
#define TRD_FF (TRD_RND + 64 * TRD_RND_STRIDE)
#define TRD_FF_CARRY 32
#define TRD_SLOT_STRIDE (TRD_FF + 64)
#define TRD_BYTES(bytes, D, n) ((D) ? TRD(bytes) + TRD_SLOT0 + (n) * TRD_SLOT_STRIDE : (bytes))
// compressions of a proof: L / 64 for a chain key, ceil((L + 9) / 64) for a final key (the padding 0x80, zeros, be64(8 (P + L)))
#define TRD_BLOCKS(D, L) ((D) == 1 ? (L) / 64 : (D) == 2 ? ((L) + 9 + 63) / 64 : 0)
static_assert(TRD_BYTES(TRK_KT_BYTES(4, TRK_ECB_BYTES(4, 1), 0), 0, 0) == TR_BLOCK0 + TR_BLOCK_STRIDE && TRD_BYTES(TRK_KT_BYTES(8, TRK_CTR_BYTES(8, 2), 2), 0, 0) == TRK_KT_BYTES(8, TRK_CTR_BYTES(8, 2), 2) &&
              TRD_BYTES(TRK_GCM_BYTES(6, 1, 2), 0, 0) == TRK_GCM_BYTES(6, 1, 2), "without a digest a trace keeps its length");
static_assert(TRD_RND == 1152 && TRD_FF == 3968 && TRD_SLOT_STRIDE == 4032 && TRD_SLOT_STRIDE % 16 == 0 && TRD_SLOT0 % 16 == 0, "the digest slot");
static_assert(TRD(TRK_ECB_BYTES(6, 1)) == TRK_ECB_BYTES(6, 1) + 8 && TRD(TRK_CTR_BYTES(4, 2)) % 16 == 0 && TRD_BYTES(TRK_ECB_BYTES(8, 4), 1, 1) % 16 == 0, "the digest region begins and ends on a multiple of 16");
static_assert(TRD_BLOCKS(1, 128) == 2 && TRD_BLOCKS(2, 55) == 1 && TRD_BLOCKS(2, 56) == 2 && TRD_BLOCKS(2, 17) == 1 && TRD_BLOCKS(0, 64) == 0, "compressions per proof");

// ---- selective disclosure: a key synthesized with the reveal flag R = 1 also proves revealed[i] = mask_i ? M[i] : 0 for a public mask chosen per proof.
// The reveal region lies BEHIND the digest region, so no offset above moves: `bytes` = the trace length with tag slots and digest region (TRD_BYTES), TRV(bytes) = that
// length rounded up to 16 is the region's base rv, and with R = 0 a trace is what it was.  For a message of L bytes:
//   rv + 0                 the mask, ceil(L / 8) bytes: bit i of the mask is bit i % 8 of byte i / 8; zero-padded to a multiple of 16
//   rv + TRV_REVEALED(L)   revealed, L bytes; zero-padded to a multiple of 16
#define TRV(bytes) (((bytes) + 15) / 16 * 16)
#define TRV_MASK 0
#define TRV_MASK_BYTES(L) (((L) + 7) / 8)
#define TRV_REVEALED(L) ((TRV_MASK_BYTES(L) + 15) / 16 * 16)
#define TRV_REGION_BYTES(L) (TRV_REVEALED(L) + ((L) + 15) / 16 * 16)
#define TRV_BYTES(bytes, R, L) ((R) ? TRV(bytes) + TRV_REGION_BYTES(L) : (bytes))
static_assert(TRV_BYTES(TRK_ECB_BYTES(4, 1), 0, 16) == TR_BLOCK0 + TR_BLOCK_STRIDE && TRV_BYTES(TRD_BYTES(TRK_KT_BYTES(8, TRK_CTR_BYTES(8, 2), 2), 2, 1), 0, 17) == TRD_BYTES(TRK_KT_BYTES(8, TRK_CTR_BYTES(8, 2), 2), 2, 1) &&
              TRV_BYTES(TRK_GCM_BYTES(6, 1, 2), 0, 17) == TRK_GCM_BYTES(6, 1, 2), "without reveal a trace keeps its length");
static_assert(TRV(TRK_ECB_BYTES(4, 1)) == TRK_ECB_BYTES(4, 1) && TRV(TRK_ECB_BYTES(6, 1)) == TRK_ECB_BYTES(6, 1) + 8 && TRV(TRK_ECB_BYTES(8, 2)) == TRK_ECB_BYTES(8, 2) + 8 && TRV(TRK_CTR_BYTES(6, 2)) % 16 == 0 &&
              TRV(TRK_CTR_BYTES(8, 1)) % 16 == 0, "the reveal region begins on a multiple of 16 for nk = 4, 6, 8");
static_assert(TRV_MASK_BYTES(1) == 1 && TRV_MASK_BYTES(17) == 3 && TRV_REVEALED(1) == 16 && TRV_REVEALED(128) == 16 && TRV_REVEALED(129) == 32 && TRV_REGION_BYTES(1) == 32 && TRV_REGION_BYTES(17) == 48 &&
              TRV_REGION_BYTES(64) == 80 && TRV_BYTES(TRK_ECB_BYTES(6, 1), 1, 16) % 16 == 0, "mask and revealed are each zero-padded to a multiple of 16");

// ---- GCM segments: a record longer than one proof is n >= 2 segment-proofs, role head / mid / tail.  A segment key's trace keeps the GCM tail's inner
// layout (the TR_GCM_* offsets) behind its AES slots -- the nb data blocks, then H, then (tail only) J_0 -- with these differences: the four bytes behind the iv hold
// ctr0, big-endian, the 32-bit counter of the segment's first data block; only a head has aad (na = 0 otherwise); the multiplications are na + nb (head), nb (mid),
// nb + 1 (tail: the last over the length block); the 16 tag bytes behind them are written by a tail only.  BEHIND the tag lies the segment region sg, 16-byte aligned:
//   sg + 0     Y_in (16): the GHASH accumulator entering the segment (mid, tail)
//   sg + 16    salt_in (16), sg + 32 salt_out (16): the salts of the commitments behind the previous segment and behind this one
//   sg + 48    the length block be64(8 A) || be64(8 L) of the whole record (16; tail)
//   sg + 64    com_in (32), sg + 96 com_out (32): the boundary commitments in SHA-256's big-endian word serialisation
//   sg + 128   per data block b, 8 bytes: the low 32 counter bits ctr0 + b mod 2^32, big-endian (4), then the carries of (ctr0 + b - 1) + 1 (4) in the CTR tail's
//              mapping: counter bit i is bit i % 8 of byte 3 - i / 8, carry bit i = 1 iff bits 0 .. i of the previous counter are all one, i <= 30
//   then, 16-byte aligned, two compression slots of TRD_SLOT_STRIDE: com_in's, com_out's (the layout of a digest slot, TRD_SCH / TRD_RND / TRD_FF)
// No offset above moves, and a lone GCM key's trace is what it was.
#define TRS_HEAD 0
#define TRS_MID 1
#define TRS_TAIL 2
#define TRS_LAST 3                                                        // digest records only (below): a mid with a byte length
#define TRS_SLOTS(role, nb) ((nb) + 1 + ((role) == TRS_TAIL ? 1 : 0))
#define TRS_GCM(nk, role, nb) ((TRK_CBC(nk, TRS_SLOTS(role, nb)) + 15) / 16 * 16)
#define TRS_MULS(role, na, nb) ((role) == TRS_HEAD ? (na) + (nb) : ((role) == TRS_MID || (role) == TRS_LAST) ? (nb) : (nb) + 1)
#define TRS_CTR0 12                                                       // inside the tail's iv slot
#define TRS_TAG(role, na, nb) (TR_GCM_MUL0(na, nb) + TRS_MULS(role, na, nb) * TR_GCM_MUL_STRIDE)
#define TRS_SEG(role, na, nb) (TRS_TAG(role, na, nb) + 16)               // sg, relative to the tail's base TRS_GCM
#define TRS_YIN 0
#define TRS_SALT_IN 16
#define TRS_SALT_OUT 32
#define TRS_LEN 48
#define TRS_COM_IN 64
#define TRS_COM_OUT 96
#define TRS_BLOCK_CTR0 128
#define TRS_BLOCK_CTR_STRIDE 8
#define TRS_BL_CTR 0
#define TRS_BL_CARRY 4
#define TRS_SLOT_IN(nb) (TRS_BLOCK_CTR0 + (TRS_BLOCK_CTR_STRIDE * (nb) + 15) / 16 * 16)
#define TRS_SLOT_OUT(nb) (TRS_SLOT_IN(nb) + TRD_SLOT_STRIDE)
#define TRS_SEG_BYTES(nb) (TRS_SLOT_OUT(nb) + TRD_SLOT_STRIDE)
#define TRS_BYTES(nk, role, na, nb) (TRS_GCM(nk, role, nb) + TRS_SEG(role, na, nb) + TRS_SEG_BYTES(nb))
// a segment proof's header, as the prover hands it to the trace kernels: iv (12), ctr0 (4, big-endian), Y_in (16), salt_in (16), salt_out (16), the length block (16),
// then the aad (head); a field its role does not use is ignored
#define TRS_HDR_IV 0
#define TRS_HDR_CTR0 12
#define TRS_HDR_YIN 16
#define TRS_HDR_SALT_IN 32
#define TRS_HDR_SALT_OUT 48
#define TRS_HDR_LEN 64
#define TRS_HDR_AAD 80
#define TRS_HDR_BYTES(A) (80 + (A))
static_assert(TRS_GCM(4, TRS_TAIL, 3) == TRK_GCM(4, 3) && TRS_GCM(8, TRS_TAIL, 2) == TRK_GCM(8, 2) && TRS_TAG(TRS_TAIL, 0, 3) == TR_GCM_TAG(0, 3), "a tail segment's AES slots and GCM tail are a lone key's without aad");
static_assert(TRS_SEG(TRS_TAIL, 0, 3) == TR_GCM_BYTES(0, 3) - TR_GCM(3) && TRS_BYTES(4, TRS_TAIL, 0, 3) == TRK_GCM_BYTES(4, 0, 3) + TRS_SEG_BYTES(3), "the segment region lies behind the GCM tail: no offset ahead of it moves");
static_assert(TRS_GCM(6, TRS_MID, 1) % 16 == 0 && TRS_SEG(TRS_HEAD, 1, 2) % 16 == 0 && TRS_SLOT_IN(1) == 144 && TRS_SLOT_IN(2) == 144 && TRS_SLOT_IN(3) == 160 && TRS_SEG_BYTES(4) % 16 == 0, "the segment region and its compression slots are 16-byte aligned");
static_assert(TRS_MULS(TRS_HEAD, 1, 4) == 5 && TRS_MULS(TRS_MID, 0, 4) == 4 && TRS_MULS(TRS_TAIL, 0, 4) == 5 && TRS_SLOTS(TRS_MID, 4) == 5 && TRS_SLOTS(TRS_TAIL, 4) == 6, "multiplications and AES slots per role");
// ---- selective disclosure on segments: a segment key synthesized with R = 1 has the reveal region of 9i (the TRV_* inner layout, for the segment's own
// len = 16 c or Lt bytes) BEHIND the segment region's two compression slots, at the next multiple of 16.  No TRS_* offset moves, and with R = 0 a trace is what it was.
// The proof's header grows by the segment's slice of the record's mask: TRS_HDR_BYTES(A) + ceil(len / 8) bytes, the mask last
#define TRS_RV(nk, role, na, nb) TRV(TRS_BYTES(nk, role, na, nb))
#define TRS_RV_BYTES(nk, role, na, nb, R, len) TRV_BYTES(TRS_BYTES(nk, role, na, nb), R, len)
#define TRS_HDR_MASK(A) TRS_HDR_BYTES(A)
#define TRS_HDR_RV_BYTES(A, R, len) (TRS_HDR_BYTES(A) + ((R) ? TRV_MASK_BYTES(len) : 0))
#define TRS_RV_ASSERT(nk) \
    static_assert(TRS_RV_BYTES(nk, TRS_HEAD, 1, 2, 0, 32) == TRS_BYTES(nk, TRS_HEAD, 1, 2) && TRS_RV_BYTES(nk, TRS_MID, 0, 1, 0, 16) == TRS_BYTES(nk, TRS_MID, 0, 1) && \
                  TRS_RV_BYTES(nk, TRS_TAIL, 0, 2, 0, 17) == TRS_BYTES(nk, TRS_TAIL, 0, 2), "without reveal a segment trace keeps its length"); \
    static_assert(TRS_RV(nk, TRS_HEAD, 1, 2) % 16 == 0 && TRS_RV(nk, TRS_MID, 0, 1) % 16 == 0 && TRS_RV(nk, TRS_TAIL, 0, 2) % 16 == 0 && TRS_RV(nk, TRS_HEAD, 1, 2) >= TRS_BYTES(nk, TRS_HEAD, 1, 2) && \
                  TRS_RV(nk, TRS_MID, 0, 1) - TRS_BYTES(nk, TRS_MID, 0, 1) < 16 && TRS_RV_BYTES(nk, TRS_TAIL, 0, 2, 1, 17) == TRS_RV(nk, TRS_TAIL, 0, 2) + 48 && \
                  TRS_RV_BYTES(nk, TRS_MID, 0, 4, 1, 64) % 16 == 0, "a segment's reveal region begins on the next multiple of 16 behind the compression slots and ends on one")
TRS_RV_ASSERT(4); TRS_RV_ASSERT(6); TRS_RV_ASSERT(8);
static_assert(TRS_HDR_RV_BYTES(13, 0, 16) == 93 && TRS_HDR_RV_BYTES(13, 1, 16) == 95 && TRS_HDR_RV_BYTES(0, 1, 17) == 83 && TRS_HDR_MASK(13) == 93, "a reveal segment header ends in the mask");
// ---- key tags on segments: a HEAD key synthesized with T = 1 or 2 key-tag blocks has the tag slots of 9e (TRK_KT_SLOT, the ordinary block-slot layout)
// BEHIND the segment region's two compression slots, slot 0 at TRK_KT(TRS_BYTES(..)), and a reveal region behind THEM, at TRV of the length with the slots.  No TRS_*
// offset moves, the proof's header is what it was (the tag comes from the key alone), and with T = 0 a trace is what it was.
#define TRS_KT(nk, role, na, nb) TRK_KT(TRS_BYTES(nk, role, na, nb))
#define TRS_KT_BYTES(nk, role, na, nb, T) TRK_KT_BYTES(nk, TRS_BYTES(nk, role, na, nb), T)
#define TRS_KT_RV(nk, role, na, nb, T) TRV(TRS_KT_BYTES(nk, role, na, nb, T))
#define TRS_KT_RV_BYTES(nk, role, na, nb, T, R, len) TRV_BYTES(TRS_KT_BYTES(nk, role, na, nb, T), R, len)
#define TRS_KT_ASSERT(nk) \
    static_assert(TRS_KT_BYTES(nk, TRS_HEAD, 1, 2, 0) == TRS_BYTES(nk, TRS_HEAD, 1, 2) && TRS_KT_RV_BYTES(nk, TRS_HEAD, 1, 2, 0, 1, 32) == TRS_RV_BYTES(nk, TRS_HEAD, 1, 2, 1, 32) && \
                  TRS_KT_RV(nk, TRS_HEAD, 1, 2, 0) == TRS_RV(nk, TRS_HEAD, 1, 2), "without key tags a segment trace keeps its length and its reveal region its place"); \
    static_assert(TRS_KT(nk, TRS_HEAD, 1, 2) % 16 == 0 && TRS_KT(nk, TRS_HEAD, 0, 1) % 16 == 0 && TRS_KT(nk, TRS_HEAD, 1, 2) >= TRS_BYTES(nk, TRS_HEAD, 1, 2) && TRK_BLOCK_STRIDE(nk) % 16 == 0 && \
                  TRS_KT_BYTES(nk, TRS_HEAD, 1, 2, 1) % 16 == 0 && TRS_KT_BYTES(nk, TRS_HEAD, 1, 2, 2) % 16 == 0 && TRS_KT_RV_BYTES(nk, TRS_HEAD, 1, 2, 2, 1, 32) % 16 == 0, \
                  "a head's tag slots begin on a multiple of 16 behind the compression slots, and the tagged stride is one"); \
    static_assert(TRS_KT_RV(nk, TRS_HEAD, 1, 2, 1) == TRS_KT(nk, TRS_HEAD, 1, 2) + TRK_BLOCK_STRIDE(nk) && TRS_KT_RV(nk, TRS_HEAD, 0, 4, 2) == TRS_KT(nk, TRS_HEAD, 0, 4) + 2 * TRK_BLOCK_STRIDE(nk), \
                  "the reveal region of a tagged head begins where the tag slots end")
TRS_KT_ASSERT(4); TRS_KT_ASSERT(6); TRS_KT_ASSERT(8);
// ---- digests on segments: a record whose segment keys were synthesized with the digest flag ends differently.  Its last data bytes lie in a segment of
// role TRS_LAST: a mid -- Y_in, com_in, com_out, nb + 1 AES slots, nb multiplications, two compression slots -- whose length is Lr = 1 .. 16 nb BYTES, the final block
// zero-padded for GHASH as a tail's.  Its tail holds no data block (nb = 0, the "closing tail"): slot 0 is H, slot 1 is J_0, its ONE multiplication runs over
// X = Y_in ^ the length block, and it has the tag and com_in.  A head, mid or last of such a record has 9f's digest region (the TRD_* inner layout) BEHIND the segment
// region's two compression slots, at the next multiple of 16: chain (D = 1) over the 16 nb bytes of a head or mid, final (D = 2) over the Lr bytes of a last.  No TRS_*
// offset moves, and without the flag a trace is what it was.
// The proof's header grows: TRS_HDR_BYTES(A), then H_in (32), then for a last be64(total_bits) and eight zero bytes -- the bit count of everything hashed up to the
// record's end, which the padding's length field takes from the header and not from the key, so that one last key serves every record whose last segment has Lr bytes
#define TRS_DG(nk, role, na, nb) TRD(TRS_BYTES(nk, role, na, nb))
#define TRS_DG_KIND(role) ((role) == TRS_LAST ? 2 : (role) == TRS_TAIL ? 0 : 1)
// a last's region ends, behind its slots, in the 16 bytes be64(total_bits) || eight zero bytes as the header gave them (the padding's length inputs)
#define TRS_DG_BITS(nblk) (TRD_SLOT0 + (nblk) * TRD_SLOT_STRIDE)
#define TRS_DG_BYTES(nk, role, na, nb, D, len) (TRD_BYTES(TRS_BYTES(nk, role, na, nb), D, TRD_BLOCKS(D, len)) + ((D) == 2 ? 16 : 0))
#define TRS_HDR_HIN(A) TRS_HDR_BYTES(A)
#define TRS_HDR_BITS(A) (TRS_HDR_BYTES(A) + 32)
#define TRS_HDR_DG_BYTES(A, D) (TRS_HDR_BYTES(A) + ((D) ? 32 : 0) + ((D) == 2 ? 16 : 0))
static_assert(TRS_MULS(TRS_HEAD, 1, 4) == 5 && TRS_MULS(TRS_MID, 0, 4) == 4 && TRS_MULS(TRS_TAIL, 0, 4) == 5 && TRS_SLOTS(TRS_HEAD, 4) == 5 && TRS_SLOTS(TRS_MID, 4) == 5 && TRS_SLOTS(TRS_TAIL, 4) == 6 &&
              TRS_BYTES(4, TRS_TAIL, 0, 3) == TRK_GCM_BYTES(4, 0, 3) + TRS_SEG_BYTES(3), "the older roles keep their slots, multiplications and lengths");
#define TRS_DG_ASSERT(nk) \
    static_assert(TRS_SLOTS(TRS_LAST, 4) == TRS_SLOTS(TRS_MID, 4) && TRS_MULS(TRS_LAST, 0, 4) == TRS_MULS(TRS_MID, 0, 4) && TRS_GCM(nk, TRS_LAST, 4) == TRS_GCM(nk, TRS_MID, 4) && \
                  TRS_TAG(TRS_LAST, 0, 4) == TRS_TAG(TRS_MID, 0, 4) && TRS_SEG(TRS_LAST, 0, 4) == TRS_SEG(TRS_MID, 0, 4) && TRS_BYTES(nk, TRS_LAST, 0, 4) == TRS_BYTES(nk, TRS_MID, 0, 4), \
                  "a last of 16 c bytes has the offsets of a mid of c"); \
    static_assert(TRS_SLOTS(TRS_TAIL, 0) == 2 && TRS_MULS(TRS_TAIL, 0, 0) == 1 && TRS_GCM(nk, TRS_TAIL, 0) % 16 == 0 && TRS_GCM(nk, TRS_TAIL, 0) >= TRK_CBC(nk, 2) && TR_GCM_V(0, 0) == 16 && \
                  TRS_TAG(TRS_TAIL, 0, 0) == 16 + 2048 + TR_GCM_MUL_STRIDE && TRS_SEG(TRS_TAIL, 0, 0) % 16 == 0 && TRS_SLOT_IN(0) == 128 && TRS_BYTES(nk, TRS_TAIL, 0, 0) % 16 == 0, \
                  "the closing tail (nb = 0) is well-formed and 16-byte aligned"); \
    static_assert(TRS_DG(nk, TRS_HEAD, 1, 4) % 16 == 0 && TRS_DG(nk, TRS_MID, 0, 4) % 16 == 0 && TRS_DG(nk, TRS_LAST, 0, 1) % 16 == 0 && TRS_DG(nk, TRS_LAST, 0, 4) >= TRS_BYTES(nk, TRS_LAST, 0, 4) && \
                  TRS_DG_BYTES(nk, TRS_MID, 0, 4, 0, 64) == TRS_BYTES(nk, TRS_MID, 0, 4) && TRS_DG_BYTES(nk, TRS_MID, 0, 4, 1, 64) == TRS_DG(nk, TRS_MID, 0, 4) + TRD_SLOT0 + TRD_SLOT_STRIDE && \
                  TRS_DG_BYTES(nk, TRS_LAST, 0, 4, 2, 56) == TRS_DG(nk, TRS_LAST, 0, 4) + TRS_DG_BITS(2) + 16 && TRS_DG_BITS(2) % 16 == 0, "a segment's digest region begins on a multiple of 16 behind the compression slots")
TRS_DG_ASSERT(4); TRS_DG_ASSERT(6); TRS_DG_ASSERT(8);
static_assert(TRS_DG_KIND(TRS_HEAD) == 1 && TRS_DG_KIND(TRS_MID) == 1 && TRS_DG_KIND(TRS_LAST) == 2 && TRS_DG_KIND(TRS_TAIL) == 0 && TRS_HDR_DG_BYTES(13, 0) == 93 && TRS_HDR_DG_BYTES(13, 1) == 125 &&
              TRS_HDR_DG_BYTES(0, 2) == 128 && TRS_HDR_HIN(0) == 80 && TRS_HDR_BITS(0) == 112, "a digest segment header: H_in behind the aad, a last's total_bits behind H_in");

// witness descriptors (one u32 per column of z)
#define WD_KIND_SHIFT 30
#define WD_BYTEBIT 0u   // [29:4] trace offset, [3:1] bit, [0] neg
#define WD_SBOX 1u      // [29:11] s-box instance, [10:1] template entry, [0] neg
#define WD_CONST 2u     // [0] value
// s-box template entry: [14:12] level, [11:4] node j at that level, [3:1] bit
