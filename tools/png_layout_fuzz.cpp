// png_layout_fuzz.cpp — the host half of the PNG pixel layouts (csrc/rtn_png_layout.h: pass geometry, filter arithmetic, pixel
// expansion; csrc/rtn_png_stream.h: the layout inspector and its blob) as a stand-alone program for a sanitizer build, the sibling of
// tools/png_stream_fuzz.cpp.  Every buffer is an exactly sized heap block, so a clean exit under -fsanitize=address,undefined means
// no position derived from file or blob bytes left its bounds.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iretinanet-for-table-detection_amd/csrc \
//       tools/png_layout_fuzz.cpp -o /tmp/png_layout_fuzz && /tmp/png_layout_fuzz 2000 page1.png page2.png ...
//
// For every file: the layout inspector on the file and on every prefix length around each chunk boundary and on 50 random prefixes,
// with an exactly sized blob; the inflate twin and the pixel twin on the valid blob; then N copies of the blob, in turn with 1 .. 3
// deflate bytes changed, the deflate data cut short, 1 .. 3 bytes of the blob's header, table and palette changed, or the blob itself
// cut short.  A copy that still passes ps_blob gets buffers sized from its own header (pages above 2^24 pixels are passed over) and
// runs both twins; a copy whose header and palette are untouched may give status 0 only with the valid file's pixels.  Prints the
// number of cases; exit status 1 on a mismatch.
#include "rtn_png_stream.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 11) % n);
}

// Both twins over one blob: 0 and the pixels, a non-zero status word, or -1 if the blob is refused or too large to try.
static long decode(const std::vector<uint8_t>& blob, uint32_t segment, std::vector<uint8_t>* pixels) {
    const PSHdr* hd = ps_blob(blob.data(), blob.size(), PL_MAGIC);
    if (!hd || (long long)hd->W * hd->H > (1ll << 24) || ps_want(hd) > (1ll << 26)) return -1;
    const size_t want = (size_t)ps_want(hd);
    std::vector<uint8_t> stream(want);
    const char* msg = "";
    int32_t st = -1;
    if (ps_inflate_host(blob.data(), blob.size(), segment, stream.data(), want, &st, &msg) != RTN_OK) { fprintf(stderr, "inflate: %s\n", msg); exit(1); }
    if (st != 0) return st;
    pixels->assign((size_t)hd->W * hd->H * 3, 0xa5);
    if (pl_pixels_host(blob.data(), blob.size(), stream.data(), want, pixels->data(), &st, &msg) != RTN_OK) { fprintf(stderr, "pixels: %s\n", msg); exit(1); }
    return st;
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s CASES file.png ...\n", argv[0]); return 2; }
    const int cases = atoi(argv[1]);
    static const uint32_t sizes[4] = {256, 1024, 4096, 1u << 20};
    long inspected = 0, mutated = 0, accepted = 0, refused = 0;
    for (int a = 2; a < argc; ++a) {
        FILE* fp = fopen(argv[a], "rb");
        if (!fp) { perror(argv[a]); return 2; }
        std::vector<uint8_t> file;
        uint8_t buf[65536];
        for (size_t n; (n = fread(buf, 1, sizeof(buf), fp)) > 0;) file.insert(file.end(), buf, buf + n);
        fclose(fp);
        char why[200];
        rtn_png_info_t info;
        std::vector<size_t> cuts;
        for (size_t pos = 8; pos + 12 <= file.size();) {
            const uint32_t len = ps_be32(file.data() + pos);
            for (int d = -1; d <= 1; ++d) cuts.push_back(pos + d);
            cuts.push_back(pos + 8);
            if ((size_t)len > file.size() - pos - 12) break;
            pos += 12 + (size_t)len;
        }
        for (int i = 0; i < 50; ++i) cuts.push_back(rnd((uint32_t)file.size()));
        for (size_t cut : cuts) {
            if (cut >= file.size()) continue;
            std::vector<uint8_t> part(file.begin(), file.begin() + cut);
            std::vector<uint8_t> blob(128 + 2 * cut);
            if (pl_inspect(part.data(), cut, 1024, &info, blob.data(), blob.size(), why, sizeof(why)) == RTN_OK) {
                fprintf(stderr, "%s: a prefix of %zu bytes was accepted\n", argv[a], cut);
                return 1;
            }
            ++inspected;
        }
        if (pl_inspect(file.data(), file.size(), 1024, &info, nullptr, 0, why, sizeof(why)) != RTN_OK) {
            fprintf(stderr, "%s: %s\n", argv[a], why);
            return 1;
        }
        std::vector<uint8_t> blob((size_t)info.blob_bytes);
        if (pl_inspect(file.data(), file.size(), 1024, &info, blob.data(), blob.size(), why, sizeof(why)) != RTN_OK) return 1;
        std::vector<uint8_t> good, out;
        for (int s = 0; s < 4; ++s)
            if (decode(blob, sizes[s], s ? &out : &good) != 0 || (s && out != good)) {
                fprintf(stderr, "%s: segment %u: the valid file did not decode\n", argv[a], sizes[s]);
                return 1;
            }
        PSHdr hd;
        memcpy(&hd, blob.data(), sizeof(hd));
        for (int i = 0; i < cases; ++i) {
            std::vector<uint8_t> m(blob);
            bool same_page = true;                                     // header, table and palette untouched
            switch (i & 3) {
            case 0:
                for (uint32_t k = 1 + rnd(3); k > 0; --k) m[hd.off_data + rnd(hd.in_bytes)] ^= (uint8_t)(1 + rnd(255));
                break;
            case 1: {
                PSHdr h2 = hd;
                h2.in_bytes = 1 + rnd(hd.in_bytes);
                h2.nsegs = (h2.in_bytes + h2.seg_bytes - 1) / h2.seg_bytes;
                memcpy(m.data(), &h2, sizeof(h2));
                break;
            }
            case 2:
                for (uint32_t k = 1 + rnd(3); k > 0; --k) m[rnd(hd.off_data - 2)] ^= (uint8_t)(1 << rnd(8));
                same_page = false;
                break;
            default:
                m.resize(rnd((uint32_t)m.size()));
                same_page = false;
            }
            const long st = decode(m, sizes[rnd(4)], &out);
            if (st == 0) {
                ++accepted;
                if (same_page && out != good) { fprintf(stderr, "%s: case %d: status 0 with other pixels\n", argv[a], i); return 1; }
            } else {
                ++refused;
            }
            ++mutated;
        }
    }
    printf("inspector prefixes %ld, mutated or cut blobs %ld (%ld decoded, %ld refused or flagged)\n", inspected, mutated, accepted, refused);
    return 0;
}
