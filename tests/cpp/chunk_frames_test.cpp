// chunk_frames_test.cpp -- crypto::batch::chunk_frames_seal / chunk_frames_open over host vectors,
// as a node's upload and receive paths would call them (Node::dispatch_upload, Node::receive_chunk).
// Three chunks (0, 1458 and 4096 bytes) are stored, framed and opened again; then frame 1 with
// one byte flipped.  Prints, per chunk, "<frame hex> <status> <ttl> <plaintext ok> <stored ok>", then
// the tampered frame's "<status> <plaintext size> <stored size> <ttl>".
#include <iostream>
#include <string>
#include <vector>

#include "ephemeralnet/crypto/Batch.hpp"

using namespace ephemeralnet;

static std::string hex(const std::vector<uint8_t>& v) {
    static const char* d = "0123456789abcdef";
    std::string s;
    for (auto b : v) { s += d[b >> 4]; s += d[b & 15]; }
    return s;
}

int main() {
    const size_t lens[3] = {0, 1458, 4096};
    std::vector<std::vector<uint8_t>> pts(3);
    std::vector<crypto::Key> ckeys(3);
    std::vector<crypto::Nonce> cnonces(3), fnonces(3);
    std::vector<ChunkId> ids(3);
    std::array<std::array<uint8_t, 32>, 2> table{};
    for (size_t k = 0; k < 2; ++k)
        for (size_t j = 0; j < 32; ++j) table[k][j] = (uint8_t)(0x40 * (k + 1) + j);
    const std::vector<uint32_t> session = {1, 0, 1}, ttl = {3600, 7, 0x01020304};
    for (size_t i = 0; i < 3; ++i) {
        pts[i].resize(lens[i]);
        for (size_t j = 0; j < lens[i]; ++j) pts[i][j] = (uint8_t)(j * 7 + 3 * i + (j >> 8));
        for (size_t j = 0; j < 32; ++j) {
            ckeys[i].bytes[j] = (uint8_t)(16 * i + j);
            ids[i][j] = (uint8_t)(0xf0 + i - 3 * j);
        }
        for (size_t j = 0; j < 12; ++j) {
            cnonces[i].bytes[j] = (uint8_t)(i + 2 * j);
            fnonces[i].bytes[j] = (uint8_t)(0x80 + i + 5 * j);
        }
    }
    std::vector<std::span<const uint8_t>> ps(pts.begin(), pts.end());
    auto stored = crypto::batch::chunk_store(ckeys, cnonces, ps, ids);
    std::vector<std::span<const uint8_t>> ds;
    std::vector<std::array<uint8_t, 32>> hashes;
    for (auto& s : stored) {
        ds.emplace_back(s.data);
        hashes.push_back(s.chunk_hash);
    }
    auto frames = crypto::batch::chunk_frames_seal(table, session, fnonces, ids, ttl, ds);
    std::vector<std::span<const uint8_t>> fs(frames.begin(), frames.end());
    auto back = crypto::batch::chunk_frames_open(table, session, fs, ids, ckeys, cnonces, hashes);
    for (size_t i = 0; i < 3; ++i)
        std::cout << hex(frames[i]) << " " << (int)back[i].status << " " << back[i].ttl_seconds << " "
                  << (back[i].plaintext == pts[i]) << " " << (back[i].stored == stored[i].data) << "\n";
    frames[1][16 + 700] ^= 0x20;
    fs.assign(frames.begin(), frames.end());
    auto bad = crypto::batch::chunk_frames_open(table, session, fs, ids, ckeys, cnonces, hashes);
    std::cout << (int)bad[1].status << " " << bad[1].plaintext.size() << " " << bad[1].stored.size() << " "
              << bad[1].ttl_seconds << " " << (int)bad[0].status << (int)bad[2].status << "\n";
    return 0;
}
