// +build gpu

// aes_gpu_peers_test.go -- NewAESPeers (aes_gpu.go): a peer table's AES objects built in one call from the
// peers' public keys and public salts, the X25519 ladders and the key derivation on the GPUs.  Each AES must
// be the one common/mapping.go:90-99 builds: NewAES over the package's own GenerateSharedSecret
// (crypto/ecdh.go:23-31) of the same values.  A packet sealed by one opens under the other, on whichever
// member owns the slot.
package crypto

import (
	"testing"
)

func TestNewAESPeersMatchesParseMapping(t *testing.T) {
	gg, err := NewGPUGroup([]int{0, 0}, 64)
	if err != nil {
		t.Fatal(err)
	}
	defer gg.Close()
	const peers = 40
	_, privKey := GenerateECKeyPair()
	_, privSalt := GenerateECKeyPair()
	pubKeys, pubSalts := make([][]byte, peers), make([][]byte, peers)
	for i := range pubKeys {
		pubKeys[i], _ = GenerateECKeyPair()
		pubSalts[i], _ = GenerateECKeyPair()
	}
	table, err := gg.NewAESPeers(pubKeys, pubSalts, privKey, privSalt)
	if err != nil || len(table) != peers {
		t.Fatalf("NewAESPeers: %d %v", len(table), err)
	}
	members := map[int]bool{}
	ip := []byte{10, 99, 0, 1}
	for i, a := range table {
		members[a.Member()] = true
		if i > 20 {
			continue // 64 slots: 40 table-built + 21 single ones
		}
		// what ParseMapping does for this peer
		one, err := gg.NewAES(GenerateSharedSecret(pubKeys[i], privKey), GenerateSharedSecret(pubSalts[i], privSalt))
		if err != nil {
			t.Fatal(err)
		}
		data := make([]byte, 1350+28)
		fillSlice(data[:1350])
		want := append([]byte(nil), data[:1350]...)
		if n, err := a.Encrypt(data, 1350, ip); err != nil || n != 1350+28 {
			t.Fatalf("peer %d: Encrypt %d %v", i, n, err)
		}
		if n, err := one.Decrypt(data, ip); err != nil || n != 1350 || string(data[:1350]) != string(want) {
			t.Fatalf("peer %d: the ParseMapping key does not open the NewAESPeers packet: %d %v", i, n, err)
		}
		if i > 0 { // and never under a neighbour's key
			if _, err := a.Encrypt(data, 1350, ip); err != nil {
				t.Fatal(err)
			}
			if _, err := table[i-1].Decrypt(data, ip); err != errOpen {
				t.Fatalf("peer %d's packet opened under peer %d's key", i, i-1)
			}
		}
	}
	if len(members) != 2 {
		t.Fatalf("the table's keys should spread over both members, got %v", members)
	}
	if _, err := gg.NewAESPeers(pubKeys[:1], pubSalts[:2], privKey, privSalt); err == nil {
		t.Fatal("public keys and salts of different number must be refused")
	}
	if _, err := gg.NewAESPeers([][]byte{make([]byte, 31)}, [][]byte{make([]byte, 32)}, privKey, privSalt); err == nil {
		t.Fatal("a 31-byte public key must be refused")
	}
	if _, err := gg.NewAESPeers(pubKeys[:1], pubSalts[:1], privKey[:31], privSalt); err == nil {
		t.Fatal("a 31-byte private key must be refused")
	}
	if out, err := gg.NewAESPeers(nil, nil, privKey, privSalt); err != nil || out != nil {
		t.Fatal("an empty table is no error")
	}
}
