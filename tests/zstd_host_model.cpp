// zstd_host_model.cpp -- a CPU decoder of .zst files through csrc/zstd_format.hpp, stage by stage
// as zstd.hip runs them (index, parse, link, decode with symbolic repeat offsets, chain, literals,
// matches, XXH64).  Test code: it proves the format constants and the parsers on the CPU (built
// with -fsanitize=address,undefined by tests/test_zstd_format.py) before the kernels run them.
//
//   zstd_host_model [--no-checksum] [--outdir DIR] FILE...
//
// prints one line per file:
//   FILE status=<first bad frame's code or 0> frames=N bad=K out=<bytes> xxh64=<hex>
//        rep=<ov1,ll>0 ov1,ll=0 ov2,ll>0 ov2,ll=0 ov3,ll>0 ov3,ll=0> fstatus=<per-frame codes>
// and writes DIR/<basename>.out (the good frames' bytes back to back) when --outdir is given.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "zstd_format.hpp"

using namespace zs;

struct Result {
    int32_t status = 0;
    std::vector<int32_t> fstatus;
    std::vector<uint8_t> out;
    uint32_t rep[6] = {0, 0, 0, 0, 0, 0};
};

static Result decode_file(const std::vector<uint8_t> &in, bool check_sum) {
    Result R;
    const uint8_t *zst = in.data();
    // frame ranges (what sdl_zstd_split_frames returns)
    std::vector<uint64_t> off{0};
    while (off.back() < in.size()) {
        FrameInfo fi;
        uint64_t bytes;
        uint32_t nb;
        const int32_t st = frame_extent(zst + off.back(), in.size() - off.back(), fi, bytes, nb);
        if (st) {  // the rest is one bad "frame"
            off.push_back(in.size());
            break;
        }
        off.push_back(off.back() + bytes);
    }
    const uint32_t nf = (uint32_t)off.size() - 1;
    std::vector<Frame> frames(nf);
    // stage 1: count, scan, fill
    uint32_t total_blocks = 0;
    for (uint32_t f = 0; f < nf; ++f) {
        frames[f].first_block = 0;
        index_frame(zst, off[f], off[f + 1], f, frames[f], nullptr, 0);
        frames[f].first_block = total_blocks;
        total_blocks += frames[f].n_blocks;
    }
    std::vector<Block> blocks(total_blocks + 1);
    for (uint32_t f = 0; f < nf; ++f) index_frame(zst, off[f], off[f + 1], f, frames[f], blocks.data(), total_blocks);
    // stage 2
    for (uint32_t b = 0; b < total_blocks; ++b) parse_block(zst, blocks[b], frames[blocks[b].frame].block_max);
    // stage 3 + arena scans
    uint64_t lit_total = 0, seq_total = 0;
    std::vector<uint64_t> lit_base(nf), seq_base(nf);
    for (uint32_t f = 0; f < nf; ++f) {
        link_frame(frames[f], blocks.data());
        lit_base[f] = lit_total;
        seq_base[f] = seq_total;
        lit_total += frames[f].lit_total;
        seq_total += frames[f].seq_total;
    }
    std::vector<uint8_t> lit(lit_total + 1);
    std::vector<SeqRec> seq(seq_total + 1);
    // stage 4
    std::vector<Tables> Tv(1);
    Tables &T = Tv[0];
    for (uint32_t b = 0; b < total_blocks; ++b) {
        Block &B = blocks[b];
        const Frame &F = frames[B.frame];
        if (F.status || B.type != 2) continue;
        block_setup_literals(zst, blocks.data(), B, T);
        block_setup_sequences(zst, blocks.data(), B, T);
        int32_t st = T.status ? T.status : T.seq_status;
        uint8_t *bl = lit.data() + lit_base[B.frame] + B.lit_base;
        if (!st) {
            if (B.sec.lit_type == 0)
                memcpy(bl, zst + B.src + B.sec.streams, B.sec.regen);
            else if (B.sec.lit_type == 1)
                memset(bl, zst[B.src + B.sec.streams], B.sec.regen);
            else
                for (uint32_t k = 0; k < 4 && !st; ++k) st = block_lit_stream(zst, B, T, k, bl);
        }
        if (!st) st = block_sequences(zst, B, T, F.block_max, seq.data() + seq_base[B.frame] + B.seq_base, R.rep);
        B.status = st;
    }
    // stage 5 + output scan
    uint64_t out_total = 0;
    for (uint32_t f = 0; f < nf; ++f) {
        chain_frame(frames[f], blocks.data());
        frames[f].out_base = (uint32_t)out_total;
        out_total += frames[f].out_size;
    }
    R.out.assign(out_total + 1, 0);
    uint8_t *out = R.out.data();
    // stage 6: literal runs, raw and RLE blocks
    for (uint32_t b = 0; b < total_blocks; ++b) {
        const Block &B = blocks[b];
        const Frame &F = frames[B.frame];
        if (F.status) continue;
        uint8_t *dst = out + F.out_base + B.out_base;
        if (B.type == 0) {
            memcpy(dst, zst + B.src, B.rsize);
        } else if (B.type == 1) {
            memset(dst, zst[B.src], B.rsize);
        } else {
            const uint8_t *bl = lit.data() + lit_base[B.frame] + B.lit_base;
            const SeqRec *rec = seq.data() + seq_base[B.frame] + B.seq_base;
            uint32_t prev_lit = 0, prev_out = 0;
            for (uint32_t i = 0; i < B.sec.nseq; ++i) {
                const uint32_t ll = rec[i].lit_end - prev_lit;
                memcpy(dst + rec[i].dst - ll, bl + prev_lit, ll);
                prev_lit = rec[i].lit_end;
                prev_out = rec[i].dst + (rec[i].ml_kind & ML_MASK);
            }
            memcpy(dst + prev_out, bl + prev_lit, B.sec.regen - prev_lit);
        }
    }
    // stage 7: matches, per frame in order
    for (uint32_t f = 0; f < nf; ++f) {
        Frame &F = frames[f];
        if (F.status) continue;
        uint8_t *fo = out + F.out_base;
        for (uint32_t i = 0; i < F.n_blocks && !F.status; ++i) {
            const Block &B = blocks[F.first_block + i];
            if (B.type != 2) continue;
            const SeqRec *rec = seq.data() + seq_base[f] + B.seq_base;
            for (uint32_t s = 0; s < B.sec.nseq; ++s) {
                const uint32_t ml = rec[s].ml_kind & ML_MASK;
                const uint32_t o = rep_resolve(RepSlot{rec[s].ml_kind >> 30, rec[s].off}, B.rep_in);
                const uint64_t pos = (uint64_t)B.out_base + rec[s].dst;
                if (o == 0 || o > pos) {
                    F.status = E_FAR;
                    break;
                }
                for (uint32_t j = 0; j < ml; ++j) fo[pos + j] = fo[pos + j - o];
            }
        }
    }
    // stage 8
    for (uint32_t f = 0; f < nf; ++f) {
        Frame &F = frames[f];
        if (F.status || F.skippable || !F.checksum || !check_sum) continue;
        if ((uint32_t)xxh64(out + F.out_base, F.out_size) != le32(zst + F.sum_off)) F.status = E_CHECKSUM;
    }
    for (uint32_t f = 0; f < nf; ++f) {
        R.fstatus.push_back(frames[f].status);
        if (frames[f].status && !R.status) R.status = frames[f].status;
    }
    // the bytes of failed frames (FAR, checksum) are undefined: report the good frames only
    std::vector<uint8_t> good;
    for (uint32_t f = 0; f < nf; ++f)
        if (!frames[f].status) good.insert(good.end(), out + frames[f].out_base, out + frames[f].out_base + frames[f].out_size);
    R.out.swap(good);  // (drops the spare byte too)
    return R;
}

int main(int argc, char **argv) {
    bool check_sum = true;
    std::string outdir;
    int rc = 0;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--no-checksum") {
            check_sum = false;
            continue;
        }
        if (a == "--outdir" && i + 1 < argc) {
            outdir = argv[++i];
            continue;
        }
        FILE *fp = fopen(a.c_str(), "rb");
        if (!fp) {
            fprintf(stderr, "%s: cannot open\n", a.c_str());
            return 2;
        }
        std::vector<uint8_t> in;
        uint8_t buf[65536];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, fp)) > 0) in.insert(in.end(), buf, buf + n);
        fclose(fp);
        Result R = decode_file(in, check_sum);
        const size_t out_len = R.out.size();
        R.out.push_back(0);  // (a non-null pointer for an empty output)
        size_t bad = 0;
        for (int32_t s : R.fstatus) bad += s != 0;
        printf("%s status=%d frames=%zu bad=%zu out=%zu xxh64=%016llx rep=%u,%u,%u,%u,%u,%u fstatus=", a.c_str(), R.status,
               R.fstatus.size(), bad, out_len, (unsigned long long)xxh64(R.out.data(), out_len), R.rep[0], R.rep[1],
               R.rep[2], R.rep[3], R.rep[4], R.rep[5]);
        for (size_t f = 0; f < R.fstatus.size(); ++f) printf("%s%d", f ? "," : "", R.fstatus[f]);
        printf("\n");
        if (!outdir.empty()) {
            const size_t slash = a.find_last_of('/');
            const std::string name = outdir + "/" + (slash == std::string::npos ? a : a.substr(slash + 1)) + ".out";
            FILE *fo = fopen(name.c_str(), "wb");
            if (!fo || fwrite(R.out.data(), 1, out_len, fo) != out_len) {
                fprintf(stderr, "%s: cannot write\n", name.c_str());
                return 2;
            }
            fclose(fo);
        }
        (void)rc;
    }
    return rc;
}
