// The byte template of an event's two pickles (tests/model_pack.py states it against pickle.dumps), as numbers: what
// pack.hip.h writes into its streams and what sign.hip.h feeds to its hashes without a stream.  One copy of every length and
// opcode group, plain constexpr values: the header compiles for the device, for the host builds of the CPU suite and for
// the thread-by-thread emulation of the pack kernels alike.
//
//   msg   = FRAME( '(' D P 'G' t_be64 'C' 0x20 pk32 0x94 't' 0x94 '.' )
//   whole = FRAME( HDR '(' D P 'G' t_be64 'C' 0x20 pk32 0x94 'C' 0x40 sig64 0x94 't' 0x94 0x81 0x94 '.' )
//   FRAME(x) = 0x80 0x04 0x95 u64le(len(x)) x
//   D    = 'N' | 'C' u8(len) data 0x94 (len < 256) | 'B' u32le(len) data 0x94 (len <= MAX_DATA)
//   P    = ')' | 'C' 0x20 sp32 0x94 'C' 0x20 op32 0x94 0x86 0x94
//
// An opcode group is packed into one 64-bit word, the byte that comes first in the stream in the lowest byte.
#pragma once

namespace tpl {

typedef unsigned long long u64;

constexpr int MAX_DATA = 60000;        // above a 64 KiB frame the pickler splits frames
constexpr int FRAME = 11;              // 0x80 0x04 0x95 and the 8-byte length
constexpr int MSG_FIXED = FRAME + 48;  // frame + '(' 'G' t 'C' 0x20 pk 0x94 't' 0x94 '.'
constexpr int WHOLE_FIXED = FRAME + 117;   // ... + 'C' 0x40 sig 0x94 and 0x81 0x94, without HDR
constexpr int PARENTS = 72;

constexpr u64 K_FRAME = 0x950480ull;           // 3 bytes: PROTO 4, FRAME
constexpr u64 K_NONE = 0x4e28ull;              // 2: '(' 'N'
constexpr u64 K_BYTES8 = 0x4328ull;            // 3: '(' 'C' and the length in byte 2
constexpr u64 K_BYTES32 = 0x4228ull;           // 6: '(' 'B' and the length in bytes 2..5
constexpr u64 K_MEMO = 0x94ull;                // 1: MEMOIZE (behind the data bytes)
constexpr u64 K_ROOT = 0x4729ull;              // 2: ')' 'G'
constexpr u64 K_ID = 0x2043ull;                // 2: 'C' 0x20
constexpr u64 K_ID_NEXT = 0x204394ull;         // 3: MEMOIZE 'C' 0x20 (between the parents)
constexpr u64 K_PARENTS_END = 0x47948694ull;   // 4: MEMOIZE TUPLE2 MEMOIZE 'G'
constexpr u64 K_MSG_END = 0x2e947494ull;       // 4: MEMOIZE 't' MEMOIZE '.'
constexpr u64 K_SIG = 0x404394ull;             // 3: MEMOIZE 'C' 0x40
constexpr u64 K_WHOLE_END = 0x2e9481947494ull; // 6: MEMOIZE 't' MEMOIZE NEWOBJ MEMOIZE '.'

// bytes of D for a data length (dl < 0: None)
constexpr int d_size(int dl) { return dl < 0 ? 1 : dl < 256 ? dl + 3 : dl + 6; }
// the bytes of an event that depend on its data and its arity (0 or 2): D and P
constexpr int var_size(int dl, int ar) { return d_size(dl) + (ar ? PARENTS : 1); }

}  // namespace tpl
